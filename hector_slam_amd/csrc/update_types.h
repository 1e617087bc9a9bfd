// update_types.h -- what the kernels of host-posed updates (map_update.h) and of device-posed ones (map_update_scans.h) share: a scan
// on a level as the passes see it, the beam geometry, the bodies of the keyed passes.  No kernel; map_update.h has the formulation.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "map_cells.h"
#include "match_types.h"
#include "update_cell_rule.h"

namespace hsm {

// What the dense line walk needs to know about ONE beam on ONE level -- the result of beam_line() and of the two divisions
// of its per-64-steps increment.  Round 3's walk derived all of this per WAVEFRONT (one beam each, 64 lanes computing the same
// numbers: ~300 of the kernel's VALU instructions per beam, twice -- the beam and its predecessor --, half of its 30 M);
// since round 4 the end-cell pass, which evaluates beam_line() per LANE anyway, stores the record and the walk reads two of
// them through the scalar cache (wave-uniform address: s_load_dwordx4 into SGPRs).
struct BeamRec {
  unsigned int abs_da;  // major-axis steps = free cells of the line; 0 = the beam is skipped (off the map, begin == end, NaN)
  unsigned int abs_db;
  unsigned int q64;     // (64 * abs_db) / abs_da: minor steps per 64 major steps ...
  unsigned int r64_oct; // ... and the remainder, << 3 | octant: bit 0 x is the major axis, bit 1 major step > 0, bit 2 minor step > 0
};

struct UpdateParams {
  LevelRW lv;
  Affine2 pose;           // Translation(mapPose.xy) * Rotation(mapPose.theta), host sinf/cosf
  const float2* pts;      // level-0 endpoints (robot frame)
  int n;
  float pt_scale;         // 2^-level (exact), DataPointContainer.h:46-58
  int bx, by;             // scanBeginMapi (OccGridMapBase.h:137)
  unsigned int serial;    // 1..kSerialMax
  float log_odds_free, log_odds_occ;
  int mark_free, mark_occ;  // currMarkFreeIndex / currMarkOccIndex (OccGridMapBase.h:123-124)
  int x0, y0, x1, y1;       // inclusive cell bounding box of everything this scan can touch
  struct BeamRec* recs;     // dense scans: one record per beam of this level (update_mark_occ_dense_kernel -> the line walk)
};

// All levels of one updateByScan in ONE launch per pass: blockIdx.y selects the level (the levels are
// independent maps, so they run concurrently and the small coarse levels hide behind level 0).
struct UpdateBatch {
  UpdateParams lv[kMaxLevels];
  int nlev;
  int stamped;  // host-side batches: a level of the batch holds restored stamps at or ahead of its marks (the apply passes' STAMPED form)
};

// geometry of beam i exactly as updateByScan / updateLineBresenhami derive it
__device__ __forceinline__ BeamLine beam_line(const UpdateParams& P, int i) {
  BeamLine b;
  const float2 p = P.pts[i];
  float ex, ey;
  affine_apply(P.pose, p.x * P.pt_scale, p.y * P.pt_scale, ex, ey);  // OccGridMapBase.h:148
  ex += 0.5f;                                                         // :151
  ey += 0.5f;
  b.x1 = (int)ex;  // cast<int>() truncation, :154
  b.y1 = (int)ey;
  const int x0 = P.bx, y0 = P.by;
  b.valid = !(x0 == b.x1 && y0 == b.y1);  // :158
  // A NaN endpoint: x86's cvttss2si makes it INT_MIN, which fails the bounds test below and drops the beam; this
  // device's conversion makes it 0, a VALID cell.  The same finite-range test the host's bounding box uses
  // (update_level) keeps both consistent with the reference; every finite coordinate it rejects fails :176-188 anyway.
  if (!(ex > -2.0f && ex < (float)P.lv.sx + 2.0f && ey > -2.0f && ey < (float)P.lv.sy + 2.0f)) b.valid = false;
  // both endpoints inside the map, :176-188
  if ((x0 < 0) || (x0 >= P.lv.sx) || (y0 < 0) || (y0 >= P.lv.sy)) b.valid = false;
  if ((b.x1 < 0) || (b.x1 >= P.lv.sx) || (b.y1 < 0) || (b.y1 >= P.lv.sy)) b.valid = false;
  const int dx = b.x1 - x0;
  const int dy = b.y1 - y0;
  const unsigned int abs_dx = (unsigned int)(dx < 0 ? -dx : dx);
  const unsigned int abs_dy = (unsigned int)(dy < 0 ? -dy : dy);
  const int offset_dx = dx > 0 ? 1 : -1;                 // util::sign, sign(0) = -1
  const int offset_dy = (dy > 0 ? 1 : -1) * P.lv.sx;
  b.start = (unsigned int)(y0 * P.lv.sx + x0);
  b.x_major = abs_dx >= abs_dy;
  if (abs_dx >= abs_dy) {  // :200-207
    b.abs_da = abs_dx;
    b.abs_db = abs_dy;
    b.offset_a = offset_dx;
    b.offset_b = offset_dy;
  } else {
    b.abs_da = abs_dy;
    b.abs_db = abs_dx;
    b.offset_a = offset_dy;
    b.offset_b = offset_dx;
  }
  b.e0 = b.abs_da / 2;
  return b;
}

// pass 1a: end cells.  One thread per beam: atomicMax leaves the FIRST beam that ends in a cell.
// Neighbouring beams end in the same cell (near walls) or in the same 32-cell bitmap word (walls along x), and
// same-address atomics serialise in L2, so each wavefront first combines what it can: of a run of adjacent lanes
// with the same end cell only the first (lowest beam index = largest key, exactly what atomicMax would keep)
// issues the atomicMax, and the bits of a run of adjacent lanes with the same bitmap word are OR-ed by a
// segmented scan so that only the first lane of the run issues the atomicOr.
__device__ __forceinline__ void mark_occ_block(const UpdateParams& P, unsigned int block) {
  const int beam = block * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (((int)(block * blockDim.x) + (int)(threadIdx.x & ~63u)) >= P.n) return;  // whole wave beyond the scan
  bool valid = beam < P.n;
  unsigned int c = 0xffffffffu;
  if (valid) {
    const BeamLine b = beam_line(P, beam);
    valid = b.valid;
    if (valid) c = (unsigned int)(b.y1 * P.lv.sx + b.x1);
  }
  const unsigned int c_prev = (unsigned int)__shfl_up((int)c, 1);
  const bool first_of_cell = valid && (lane == 0 || c_prev != c);
  if (first_of_cell) atomicMax(&P.lv.key_occ[c], (P.serial << kBeamBits) | (kBeamMask - (unsigned int)beam));
  // bitmap: runs of adjacent valid lanes with the same word
  const unsigned int w = valid ? (c >> 5) : (0xfffffff0u - (unsigned int)lane);  // invalid lanes never join a run
  const unsigned int w_prev = (unsigned int)__shfl_up((int)w, 1);
  const bool head = lane == 0 || w_prev != w;
  const unsigned long long heads = __ballot(head);
  unsigned int m = valid ? (1u << (c & 31u)) : 0u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned int up = (unsigned int)__shfl_down((int)m, d);
    // lanes lane+1 .. lane+d belong to this lane's run iff none of them starts a new one
    const bool same = (lane + d < 64) && (((heads >> (lane + 1)) & ((1ull << d) - 1ull)) == 0ull);
    if (same) m |= up;
  }
  if (head && valid) atomicOr(&P.lv.occ_bits[w], m);
}

// dense scans: "a beam ends here" is bit 1 of the cell's mark byte instead of a bit of the row-major end-cell bitmap
constexpr unsigned char kMarkCrossed = 1, kMarkEnd = 2;

// pass 1b: line cells.  WHICH beam crossed a cell first only matters where some beam also ENDS (the
// free-then-occupied revert, OccGridMapBase.h:231-233); everywhere else "some beam of this scan crossed
// it" is all the apply pass needs (the serial tag; the beam index only where a beam ends).  This walk
// serves the scans below 4096 beams, where the whole update is launch-latency bound: every crossed cell
// takes the atomicMax of the full key, end cell or not, so the pass does not read the end-cell bitmap and
// does not depend on pass 1a -- both run in ONE launch (update_mark_kernel).
__device__ __forceinline__ void mark_free_block(const UpdateParams& P, unsigned int block) {
  const int lane = threadIdx.x & 63;
  const int beam = block * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (beam >= P.n) return;
  const BeamLine b = beam_line(P, beam);
  if (!b.valid) return;
  const unsigned int key = (P.serial << kBeamBits) | (kBeamMask - (unsigned int)beam);
  if ((unsigned int)lane >= b.abs_da) return;
  // Lane k visits steps k, k+64, ...: instead of one integer division per step (line_cell), carry the
  // quotient/remainder of (e0 + i*db) / da forward by the per-64-step increment -- two divisions per lane.
  const unsigned int num0 = b.e0 + (unsigned int)lane * b.abs_db;
  unsigned int q = num0 / b.abs_da, r = num0 - q * b.abs_da;
  const unsigned int inc = 64u * b.abs_db;
  const unsigned int q64 = inc / b.abs_da, r64 = inc - q64 * b.abs_da;
  const unsigned int step_a = (unsigned int)(64 * b.offset_a);
  unsigned int base = b.start + (unsigned int)(lane * b.offset_a);
  const bool x_major = b.x_major;
  // Duplicate suppression.  Neighbouring beams of a dense scan run through the SAME cells for their first
  // hundreds of steps (all lines start in the same cell and separate by less than a cell until 1/dtheta
  // cells out).  If beam-1 is valid, lies in the same octant and visits the same cell at step i, it writes
  // the same tag there -- or, on an end cell, a LARGER key (lower beam index) -- so this beam's access is
  // redundant and is skipped; by induction the lowest-indexed beam of each run does the write.
  const BeamLine pb = beam > 0 ? beam_line(P, beam - 1) : b;
  const bool dedup = beam > 0 && pb.valid && pb.offset_a == b.offset_a && pb.offset_b == b.offset_b;
  const unsigned int pnum0 = pb.e0 + (unsigned int)lane * pb.abs_db;
  unsigned int pq = dedup ? pnum0 / pb.abs_da : 0u, pr = dedup ? pnum0 - pq * pb.abs_da : 0u;
  const unsigned int pinc = 64u * pb.abs_db;
  const unsigned int pq64 = dedup ? pinc / pb.abs_da : 0u, pr64 = dedup ? pinc - pq64 * pb.abs_da : 0u;
  for (unsigned int i = lane; i < b.abs_da; i += 64) {  // abs_da free cells: steps 0 .. abs_da-1
    if (!(dedup && i < pb.abs_da && pq == q)) {
      const unsigned int c = base + (unsigned int)((int)q * b.offset_b);  // == line_cell(b, i)
      // the same cell as (x, y): i steps along the major axis, q along the minor one
      const int sa = b.offset_a > 0 ? (int)i : -(int)i, sb = b.offset_b > 0 ? (int)q : -(int)q;
      const unsigned int cx = (unsigned int)(P.bx + (x_major ? sa : sb)), cy = (unsigned int)(P.by + (x_major ? sb : sa));
      const unsigned int kc = key_free_index(P.lv, cx, cy);
      atomicMax(&P.lv.key_free[kc], key);
    }
    base += step_a;
    q += q64;
    r += r64;
    if (r >= b.abs_da) {
      r -= b.abs_da;
      ++q;
    }
    pq += pq64;
    pr += pr64;
    if (dedup && pr >= pb.abs_da) {
      pr -= pb.abs_da;
      ++pq;
    }
  }
}

// SCATTER_TEXELS (quad layout): the cell's new probability goes straight into the four texels it is a
// corner of -- component 0 of texel (x,y), 1 of (x-1,y), 2 of (x,y-1), 3 of (x-1,y-1), with update_texels_kernel's
// edge replication at the last column / row -- so the texel pass and its launch disappear.  Every texel component
// has exactly one writer (the thread of its cell), untouched components keep their value: same bits as the rebuild.
__device__ __forceinline__ void scatter_texels(const LevelRW& lv, int x, int y, float p) {
  float* q = reinterpret_cast<float*>(lv.quad);
  const int sx = lv.sx, sy = lv.sy;
  const bool lastx = x == sx - 1, lasty = y == sy - 1;
  auto put = [&](int tx, int ty, int comp) { q[4 * (size_t)quad_index(tx, ty, lv.tiles_x, sx) + comp] = p; };
  put(x, y, 0);
  if (x > 0) put(x - 1, y, 1);
  if (lastx) put(x, y, 1);
  if (y > 0) put(x, y - 1, 2);
  if (lasty) put(x, y, 2);
  if (x > 0 && y > 0) put(x - 1, y - 1, 3);
  if (lastx && y > 0) put(x, y - 1, 3);
  if (lasty && x > 0) put(x - 1, y, 3);
  if (lastx && lasty) put(x, y, 3);
}

// dense over the box [x0..x1] x [y0..y1]: bresenhamCellFree / bresenhamCellOcc (OccGridMapBase.h:216-241, update_cell_rule.h)
//
// "A beam of THIS scan ends here" is the cell's bit in the end-cell bitmap (set by mark_occ_block,
// cleared here), so the occ-key plane is only read where the bit is set -- end cells are walls, and most of that
// plane's cache lines are never touched by this pass.  The bitmap word is cleared by the lane of its first cell;
// that is only safe when every reader of a word sits in the SAME wavefront (reads program-ordered before the
// store), which holds when rows are a multiple of 64 cells: the pass then runs over the box widened to 64-cell
// column boundaries (the extra cells carry no key of this scan).  Other map widths keep the plain form.
// The body of update_apply_kernel and of update_apply_scan_kernel; grid-stride: `first` is this thread's first cell of the
// box, `stride` the number of threads in the grid (computed by the kernels, where blockDim is a compile-time-uniform read).
// STAMPED (restored levels, see the header): the stored stamp is read, with the log-odds, and the reference's tests on it are applied.
template <bool SCATTER_TEXELS, bool STAMPED>
__device__ __forceinline__ void apply_box(const UpdateParams& P, size_t first, size_t stride) {
  if (P.x1 < P.x0) return;  // this level has nothing to apply
  const bool aligned = (P.lv.sx & 63) == 0;
  const int bx0 = aligned ? (P.x0 & ~63) : P.x0;
  const int w = aligned ? ((P.x1 | 63) - bx0 + 1) : (P.x1 - P.x0 + 1), h = P.y1 - P.y0 + 1;
  const size_t n = (size_t)w * h;
  for (size_t t = first; t < n; t += stride) {
    const int x = bx0 + (int)(t % (size_t)w), y = P.y0 + (int)(t / (size_t)w);
    const size_t c = (size_t)y * P.lv.sx + x;
    const unsigned int kf = P.lv.key_free[key_free_index(P.lv, (unsigned int)x, (unsigned int)y)];
    unsigned int ko;
    bool occ;
    if (aligned) {
      const unsigned int word = P.lv.occ_bits[c >> 5];
      occ = (word >> (c & 31u)) & 1u;
      ko = occ ? P.lv.key_occ[c] : 0u;
      occ = occ && (ko >> kBeamBits) == P.serial;  // (a bit without this scan's key cannot occur; cheap to insist)
      if (word != 0u && (c & 31u) == 0) P.lv.occ_bits[c >> 5] = 0u;
    } else {
      // every set bit lies inside the box, so zeroing each word that overlaps it is exact
      if ((c & 31u) == 0 || x == P.x0) P.lv.occ_bits[c >> 5] = 0u;
      ko = P.lv.key_occ[c];
      occ = (ko >> kBeamBits) == P.serial;
    }
    const bool fre = (kf >> kBeamBits) == P.serial;
    if (!fre && !occ) continue;
    const CellUpdate u = update_cell_rule<STAMPED>(P.lv.logodds[c], STAMPED ? P.lv.update_index[c] : 0, occ, fre,
                                                   kBeamMask - (ko & kBeamMask), kBeamMask - (kf & kBeamMask), P.log_odds_free,
                                                   P.log_odds_occ, P.mark_free, P.mark_occ);
    if (!u.written) continue;
    P.lv.logodds[c] = u.logodds;
    P.lv.update_index[c] = u.stamp;
    const float p = grid_probability(u.logodds);
    P.lv.prob[c] = p;
    if (SCATTER_TEXELS) scatter_texels(P.lv, x, y, p);
  }
}

}  // namespace hsm
