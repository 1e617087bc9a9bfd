// map_update.h -- log-odds map update (updateByScan) and probability-texel maintenance
// as gfx950 HIP kernels.
//
// Reference: OccGridMapBase::updateByScan + updateLineBresenhami / bresenham2D /
// bresenhamCellFree / bresenhamCellOcc, HSL/map/OccGridMapBase.h:121-260, cell rules
// GridMapLogOdds.h:135-156.  Net effect per scan and per cell:
//   * a cell that is the END cell of any non-skipped beam gets the occupied update,
//     at most once; otherwise a cell crossed by any beam gets the free update, once;
//   * if (in beam order) a free touch came BEFORE the first occupied touch, the
//     reference first applies and then reverts the free update, so the float result
//     is ((l + f) - f) [+ o] instead of l [+ o].  That rounding artefact is reproduced.
//
// Parallel formulation (bit-exact with the sequential reference):
//   pass 1 "mark" (per beam): (a) every beam atomicMax'es
//       key = (scan serial << 20) | (0xFFFFF - beam index) into the occ-key plane at its end cell,
//       which leaves the FIRST beam (lowest index) ending there; (b) one wavefront per beam, lane k
//       owns Bresenham steps k, k+64, ... -- the cell of step i has a closed form (minor steps =
//       floor((e0 + i*db)/da)), so no lane walks the line sequentially -- and tags every crossed
//       cell in the free-key plane with an atomicMax of the key (lowest crossing beam index, needed
//       for the revert artefact where a beam also ends).  Dense scans mark one byte per crossed
//       cell instead (see below).
//   pass 2 "apply" (per cell, DENSE over the bounding box of the scan):  every cell whose keys
//       carry the current serial applies the reference's rule -- occupied if any beam ends there
//       (after undoing the free update when a lower-indexed beam crossed it first), else free --
//       to the log-odds plane, writes the reference's updateIndex stamp and the new probability.
//       Rows are contiguous, so all loads and stores are coalesced; no float atomics, no races.
//   pass 3 "texels" (per cell, dense over the box grown by one):  rebuilds the float4 texels
//       {P(x,y),P(x+1,y),P(x,y+1),P(x+1,y+1)} the matcher samples.
// Keys of earlier scans are always smaller than the current ones, so the key planes never need
// clearing (only when the 12-bit serial wraps, every 4095 updates).
//
// Stored stamps.  The reference's two cell rules test the cell's stored updateIndex against the scan's marks F = counter + 1
// and O = counter + 2 (:218, :228).  Every stamp the kernels write lies below the counter of the next scan, so the tests always
// pass and the apply passes need not read the plane -- until hsm_upload_level restores a level whose stamps are at or ahead of
// the counter.  Then, with s the stamp in front of the scan: s >= O, nothing is written (log-odds, stamp, probability and
// texels stay); s == F, a crossing writes nothing and an end applies unsetFree (l -= f, whether or not the scan crossed the
// cell first), then the occupied update, stamp O; s < F, the rule above.  The apply passes have a STAMPED instantiation that
// loads the stamp and does exactly that (the marks and bitmap words of skipped cells are cleared as for any other cell); the
// host selects it per call while Level::uploaded_stamp_max is ahead of the level's counter, so the hot path never pays the
// extra 4 B per touched cell (profiles/r16/README.md).  tests/test_gpu_restored_stamps.py.
//
// Traffic: mark = one 4-byte load (+ rarely an atomic) per visited cell; apply = 12 B
// read + 12 B written per touched cell of the box; texels = 16 B written per cell of the box.
// HBM/L2-bound integer/byte work, no MFMA.
#pragma once
#include <hip/hip_runtime.h>

#include "beam_sample.h"
#include "libm_exact.h"
#include "map_cells.h"
#include "match_types.h"
#include "update_gate.h"

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

// pass 1a of a dense scan: the occ key as above; the end-cell flag goes into the cell's MARK BYTE (value 2)
// -- the byte the line walk of pass 1b reads and writes anyway, in the same tiled plane -- and the bitmap is not touched.
// All writers of a byte store the same value; the launch boundary orders them before pass 1b.
__global__ void __launch_bounds__(256) update_mark_occ_dense_kernel(const UpdateBatch B) {
  const UpdateParams& P = B.lv[blockIdx.y];
  const int beam = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (((int)(blockIdx.x * blockDim.x) + (int)(threadIdx.x & ~63u)) >= P.n) return;  // whole wave beyond the scan
  bool valid = beam < P.n;
  unsigned int c = 0xffffffffu, kc = 0u;
  if (valid) {
    const BeamLine b = beam_line(P, beam);
    valid = b.valid;
    BeamRec rec = {0u, 0u, 0u, 0u};
    if (valid) {
      c = (unsigned int)(b.y1 * P.lv.sx + b.x1);
      kc = mark_index(P.lv, (unsigned int)b.x1, (unsigned int)b.y1);
      // the walk's per-64-steps increment of (e0 + i * db) / da: quotient and remainder (abs_da >= 1 for a valid beam)
      const unsigned int inc = 64u * b.abs_db;
      const unsigned int q64 = inc / b.abs_da;
      const bool major_pos = b.offset_a > 0, minor_pos = b.offset_b > 0;
      rec.abs_da = b.abs_da;
      rec.abs_db = b.abs_db;
      rec.q64 = q64;
      rec.r64_oct = ((inc - q64 * b.abs_da) << 3) | (b.x_major ? 1u : 0u) | (major_pos ? 2u : 0u) | (minor_pos ? 4u : 0u);
    }
    reinterpret_cast<uint4*>(P.recs)[beam] = make_uint4(rec.abs_da, rec.abs_db, rec.q64, rec.r64_oct);
  }
  const unsigned int c_prev = (unsigned int)__shfl_up((int)c, 1);
  if (valid && (lane == 0 || c_prev != c)) {  // of a run of adjacent lanes with the same end cell the first = lowest beam index
    atomicMax(&P.lv.key_occ[c], (P.serial << kBeamBits) | (kBeamMask - (unsigned int)beam));
    P.lv.free_bytes[kc] = kMarkEnd;
    P.lv.free_bytes[mark_tile_end_offset(P.lv.sx, P.lv.sy) + (kc >> 7)] = 1;
  }
}

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

// passes 1a + 1b of a SMALL scan in one launch: the first occ_blocks workgroups of a row mark the end cells, the rest
// walk the lines with keyed atomics (no dependency between the two, see mark_free_block)
__global__ void __launch_bounds__(256) update_mark_kernel(const UpdateBatch B, unsigned int occ_blocks) {
  const UpdateParams& P = B.lv[blockIdx.y];
  if (blockIdx.x < occ_blocks)
    mark_occ_block(P, blockIdx.x);
  else
    mark_free_block(P, blockIdx.x - occ_blocks);
}

// dense over the box [x0..x1] x [y0..y1]: bresenhamCellFree / bresenhamCellOcc (OccGridMapBase.h:216-241)
//
// "A beam of THIS scan ends here" is the cell's bit in the end-cell bitmap (set by mark_occ_block,
// cleared here), so the occ-key plane is only read where the bit is set -- end cells are walls, and most of that
// plane's cache lines are never touched by this pass.  The bitmap word is cleared by the lane of its first cell;
// that is only safe when every reader of a word sits in the SAME wavefront (reads program-ordered before the
// store), which holds when rows are a multiple of 64 cells: the pass then runs over the box widened to 64-cell
// column boundaries (the extra cells carry no key of this scan).  Other map widths keep the plain form.
// SCATTER_TEXELS (quad layout): the cell's new probability goes straight into the four texels it is a
// corner of -- component 0 of texel (x,y), 1 of (x-1,y), 2 of (x,y-1), 3 of (x-1,y-1), with update_texels_kernel's
// edge replication at the last column / row -- so the texel pass and its launch disappear.  Every texel component
// has exactly one writer (the thread of its cell), untouched components keep their value: same bits as the rebuild.
// The body of update_apply_kernel and of update_apply_scan_kernel; grid-stride: `first` is this thread's first cell of the
// box, `stride` the number of threads in the grid (computed by the kernels, where blockDim is a compile-time-uniform read).
// STAMPED (restored levels, see the header): the cell's stored stamp is read and the reference's tests on it are applied.
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
    bool stored_free = false;  // the stored stamp IS this scan's free mark: no free update, unsetFree in front of the occupied one
    if (STAMPED) {
      const int s = P.lv.update_index[c];
      if (s >= P.mark_occ) continue;  // :228 fails, and :218 with it: the cell stays as it is
      stored_free = s == P.mark_free;
      if (stored_free && !occ) continue;  // :218 fails
    }
    float l = P.lv.logodds[c];
    int stamp;
    if (occ) {
      // free-touched by an earlier beam of this scan: applied, then reverted (:231-233)
      // (in fp32 (l + f) - f == l unless l + f leaves l's binade, so this comparison shows in the bits only for cells just above
      // -2, -4, -8 ...: tests/test_gpu_update_order.py puts cells there and runs scans in several beam orders)
      if (stored_free) {
        l -= P.log_odds_free;
      } else if (fre && (kBeamMask - (kf & kBeamMask)) < (kBeamMask - (ko & kBeamMask))) {
        l += P.log_odds_free;
        l -= P.log_odds_free;
      }
      if (l < 50.0f) l += P.log_odds_occ;  // updateSetOccupied
      stamp = P.mark_occ;
    } else {
      l += P.log_odds_free;                // updateSetFree
      stamp = P.mark_free;
    }
    P.lv.logodds[c] = l;
    P.lv.update_index[c] = stamp;
    const float p = grid_probability(l);
    P.lv.prob[c] = p;
    if (SCATTER_TEXELS) {
      float* q = reinterpret_cast<float*>(P.lv.quad);
      const int sx = P.lv.sx, sy = P.lv.sy;
      const bool lastx = x == sx - 1, lasty = y == sy - 1;
      auto put = [&](int tx, int ty, int comp) { q[4 * (size_t)quad_index(tx, ty, P.lv.tiles_x, sx) + comp] = p; };
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
  }
}

template <bool SCATTER_TEXELS, bool STAMPED>
__global__ void __launch_bounds__(256) update_apply_kernel(const UpdateBatch B) {
  apply_box<SCATTER_TEXELS, STAMPED>(B.lv[blockIdx.y], blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}


// ---- dense scans (>= HSM_MERGED_MARK_MAX beams): one BYTE per crossed cell instead of a key -------------------------------
// Measured on the 16 k-beam scans of configs[4] (profiles/r03/README.md): the keyed form moves 4.7x the algorithmic bytes
// -- the line walk writes a 4-byte tag per crossed cell and the dense apply pass reads a 4-byte key for EVERY cell of the
// bounding box (2x the touched cells).  WHICH beam crossed a cell first only matters where a beam also ends (see
// mark_free_block); everywhere else "crossed by this scan" is all there is to say.
//   update_mark_occ_dense_kernel: the occ key of an end cell, and the value 2 in its mark byte ("a beam ends here").
//   update_mark_free_dense_kernel: mark_free_block's walk (one wavefront per beam, lane k owns steps k, k+64, ...; duplicate
//     suppression against the previous beam) on ONE byte per crossed cell -- a quarter of the bytes, and consecutive lanes
//     touch consecutive bytes of a tile row.  A step loads the byte: flagged as an end cell, it takes the keyed atomicMax as
//     before; already 1, nothing; else it stores 1.  All writers store the same value: a benign race.  (A bitmap with one
//     atomicOr per tile and lane -- lane k walking 8 consecutive steps -- was built first: 354 us against 110, every lane's
//     accesses land in a different line.  The end-cell flag first lived in the row-major bitmap of the keyed path: up to 64
//     lines per access for a y-major beam, and four more words per lane in the apply pass.)
//   update_apply_dense_kernel: one wavefront per 32 x 8-cell block of the box (2 tiles = 256 contiguous bytes of the byte
//     map).  It reads the block's bytes, skips the block when all are zero, applies the reference's rule to the marked
//     cells row by row (coalesced 128-byte row segments), and clears what it read -- the block has ONE owner, so there is no race
//     on the marks, and the byte map is all zero again between updates (no generation tag to wrap).  Untouched cells cost
//     1 byte instead of 4 bytes + 1 bit.
// Same cells, same rule, same order-dependent artefacts: the maps stay bit-identical to the reference.
#ifndef HSM_MARK_XCD_CHUNK  // workgroups of consecutive beams per XCD turn (xcd_block); < 0: the hardware's round robin
#define HSM_MARK_XCD_CHUNK 16
#endif

// a wave-uniform kernel argument pinned in SGPRs before a loop (left alone, the compiler re-loads it from the kernarg segment
// -- s_load + s_waitcnt -- inside every conditional block of every iteration)
template <class T>
__device__ __forceinline__ T pinned_sgpr(T v) {
  asm volatile("" : "+s"(v));
  return v;
}

// What bounds this kernel was measured (profiles/r03/README.md, what-if builds): with NO memory operation in the walk it
// still took 50 of its 77 us -- instruction issue, not HBM, L2 atomics or load latency (unrolling the walk for four loads in
// flight, several beams per wavefront, plain stores instead of the atomics: no gain).  So the walk is kept short: the cell
// coordinates advance incrementally (no multiplications: v_mad_u64_u32 / v_mul_lo_u32 are quarter rate), the tile row
// offset is a 24-bit multiply, the kernel arguments sit in SGPRs, the per-beam divisions are float reciprocals with an
// exact fix-up (every operand is below 2^24).
__device__ __forceinline__ unsigned int div_small(unsigned int num, unsigned int den) {  // num, den < 2^24, den > 0: exact
  unsigned int q = (unsigned int)(__builtin_amdgcn_rcpf((float)den) * (float)num);
  // the estimate is within one of the quotient
  int rem = (int)(num - q * den);
  if (rem < 0) {
    --q;
    rem += (int)den;
  }
  if (rem >= (int)den) ++q;
  return q;
}

__host__ __device__ __forceinline__ int mark_dense_blocks(int n) {  // workgroups of 4 wavefronts = 4 beams, a multiple of 8
  return ((n + 3) / 4 + 7) / 8 * 8;
}

// Tried in round 4 and dropped (profiles/r04/update_variants_kernel_us.txt, maps bit-identical in every variant): G = 2 / 4
// beams side by side in one wavefront, 64 / G lanes each (the set-up amortised over G beams): 76.8 / 120 us against 72.1 --
// the beams of a group differ in length and octant, so lanes idle and the loop diverges; without the duplicate suppression:
// 104 us -- the per-step load only sees marks that have reached this XCD's L2, the predecessor test
// needs no memory at all.
__global__ void __launch_bounds__(256) update_mark_free_dense_kernel(const UpdateBatch B) {
  const UpdateParams& P = B.lv[blockIdx.y];
  const int lane = threadIdx.x & 63;
  // Neighbouring beams cross the same cells for most of their length, and a mark byte read from another XCD's L2 is stale
  // (this kernel's stores stay in the writer's L2 until they are evicted): with the hardware's round robin of workgroups
  // over the XCDs every XCD walks every part of the fan.  Chunks of consecutive workgroups per XCD (the grid's x extent is
  // a multiple of 8, so workgroup b of any level runs on XCD b % 8) keep a sector's lines in ONE L2, where the walk sees
  // its neighbours' marks and skips the stores.
  const int wg = HSM_MARK_XCD_CHUNK >= 0 ? xcd_block((int)blockIdx.x, (int)gridDim.x, HSM_MARK_XCD_CHUNK) : (int)blockIdx.x;
  const int beam = __builtin_amdgcn_readfirstlane(wg * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6));  // wave-uniform
  if (beam >= P.n) return;
  // the beam's record and its predecessor's: wave-uniform 16-byte loads (scalar cache), everything derived from them
  // stays in SGPRs
  const uint4* __restrict__ recs = reinterpret_cast<const uint4*>(P.recs);
  const uint4 rb = recs[beam];
  const unsigned int da = rb.x;
  if (da == 0u) return;  // skipped beam (beam_line: invalid)
  if ((unsigned int)lane >= da) return;
  const uint4 rp = beam > 0 ? recs[beam - 1] : make_uint4(0u, 0u, 0u, 0u);
  const unsigned int db = rb.y, q64 = rb.z, r64 = rb.w >> 3, oct = rb.w & 7u;
  const unsigned int key = (P.serial << kBeamBits) | (kBeamMask - (unsigned int)beam);
  // lane k visits steps k, k + 64, ...: quotient / remainder of (e0 + i*db) / da carried forward by the per-64-steps increment
  const bool small = da < (1u << 17);  // (e0 + 63 db, 64 db < 2^24: always, for maps below 131072 cells a side)
  const unsigned int num0 = (da >> 1) + (unsigned int)lane * db;  // e0 = abs_da / 2
  unsigned int q = small ? div_small(num0, da) : num0 / da;
  unsigned int r = num0 - q * da;
  // duplicate suppression against the previous beam (mark_free_block): valid, same octant
  const bool dedup = rp.x != 0u && (rp.w & 7u) == oct;
  const unsigned int pda = dedup ? rp.x : 0u;  // no step is "also the previous beam's" without dedup
  const unsigned int pden = dedup ? rp.x : 1u, pdb = rp.y;
  const unsigned int pnum0 = (pden >> 1) + (unsigned int)lane * pdb;
  unsigned int pq = dedup ? (pden < (1u << 17) ? div_small(pnum0, pden) : pnum0 / pden) : 0u, pr = dedup ? pnum0 - pq * pden : 0u;
  const unsigned int pq64 = dedup ? rp.z : 0u, pr64 = dedup ? rp.w >> 3 : 0u;
  // the walk in (x, y): i steps along the major axis, q along the minor one; both advance by additions
  const bool x_major = (oct & 1u) != 0u;
  const int sgn_a = (oct & 2u) ? 1 : -1, sgn_b = (oct & 4u) ? 1 : -1;
  const int ax = x_major ? sgn_a : 0, ay = x_major ? 0 : sgn_a, mx = x_major ? 0 : sgn_b, my = x_major ? sgn_b : 0;
  int cx = P.bx + ax * lane + mx * (int)q, cy = P.by + ay * lane + my * (int)q;
  const int dx64 = 64 * ax + mx * (int)q64, dy64 = 64 * ay + my * (int)q64;  // per iteration, before the remainder's carry
  const unsigned int tiles_x = pinned_sgpr((unsigned int)P.lv.kf_tiles_x);
  // (global address space spelled out: a pointer that went through pinned_sgpr's asm is a generic one to the compiler, and the
  // walk's byte accesses became flat_load / flat_store with 64-bit per-lane addresses instead of global_* on an SGPR base)
  typedef __attribute__((address_space(1))) unsigned char gbyte;
  typedef __attribute__((address_space(1))) unsigned int gword;
  gbyte* const marks = (gbyte*)pinned_sgpr(P.lv.free_bytes);
  gword* const keys = (gword*)pinned_sgpr(P.lv.key_free);
  const unsigned int mtiles_x = pinned_sgpr((unsigned int)mark_tiles_x(P.lv.sx));
  auto key_index = [&]() -> unsigned int {  // of the current cell, in the free-key plane
    return ((__umul24((unsigned int)cy >> 2, tiles_x) + ((unsigned int)cx >> 3)) << 5) | (((unsigned int)cy & 3u) << 3) |
           ((unsigned int)cx & 7u);  // == key_free_index(P.lv, cx, cy): rows of tiles and tiles per row are below 2^24
  };
  auto cell_index = [&]() -> unsigned int {  // of the current cell, in the mark-byte plane
    return ((__umul24((unsigned int)cy >> 3, mtiles_x) + ((unsigned int)cx >> 4)) << 7) | (((unsigned int)cy & 7u) << 4) |
           ((unsigned int)cx & 15u);  // == mark_index(P.lv, cx, cy)
  };
  auto advance = [&]() {  // 64 steps on: the carries of both error accumulators
    q += q64;
    r += r64;
    cx += dx64;
    cy += dy64;
    if (r >= da) {
      r -= da;
      ++q;
      cx += mx;
      cy += my;
    }
    pq += pq64;
    pr += pr64;
    if (pr >= pda && dedup) {
      pr -= pda;
      ++pq;
    }
  };
  auto touch = [&](unsigned int kc, unsigned char m, unsigned int kkey) {  // kkey: the cell's index in the free-key plane
    if (m & kMarkEnd) {
      atomicMax((unsigned int*)&keys[kkey], key);  // a beam ends here: the lowest crossing beam index matters (revert artefact)
    } else if (m == 0) {            // (a stale 0 only repeats the store)
      marks[kc] = kMarkCrossed;
    }
  };
  // (two steps per iteration with both byte loads in flight before either is acted on: no gain, see above)
  const gbyte* const tile_end = (const gbyte*)pinned_sgpr(P.lv.free_bytes + mark_tile_end_offset(P.lv.sx, P.lv.sy));
  for (unsigned int i = lane; i < da; i += 64) {  // abs_da free cells: steps 0 .. abs_da-1
    if (!(i < pda && pq == q)) {
      const unsigned int kc = cell_index();
      if (tile_end[kc >> 7] == 0) {
        marks[kc] = kMarkCrossed;  // no beam ends in this tile: nothing to look at (an already set mark is stored again)
      } else {
        // one byte load from the line the store goes to (the row-major end-cell bitmap cost a y-major beam 64 lines per access)
        touch(kc, marks[kc], key_index());
      }
    }
    advance();
  }
}

// The dense apply pass: one wavefront per 32 x 8-cell block of the box (two 16 x 8 mark tiles = 256 contiguous mark bytes, one
// dword per lane); the box is widened to block boundaries, any map width (the tile rows are padded to whole blocks).  A
// wavefront's blocks are a chain of memory round trips (marks -> log-odds rows -> stores), a dozen blocks long, and the pass was
// waiting for them 84 % of the time (profiles/r03/README.md).  So the marks of the NEXT block are requested before this one is
// processed, and the rows of a block are all requested before the first is computed.
// Lane l works on column l % 32 of the block and on rows 2 i + l / 32 (i = 0 .. 3): every access of the log-odds /
// stamp / probability planes is two 128-byte row segments per wavefront.  A block is skipped when no mark is set; else the
// reference's rule on the marked cells, marks cleared.  The three planes are written with non-temporal stores -- 12 bytes per
// touched cell that nothing reads again before the next update; kept out of the L2 they leave it to the marks and the log-odds
// rows (update 0.198 -> 0.178 ms on configs[4]; non-temporal LOADS of the rows or stores of the cleared marks lose: 0.205 ms).
// (Measured against 64 x 4-cell blocks on the 8 x 4 tiling: profiles/r04/README.md 20.)
template <bool SCATTER_TEXELS, bool STAMPED>
__global__ void __launch_bounds__(256) update_apply_dense_kernel(const UpdateBatch B) {
  const UpdateParams& P = B.lv[blockIdx.y];
  if (P.x1 < P.x0) return;
  const int lane = threadIdx.x & 63;
  const int xl = lane & 31, rh = lane >> 5;
  const int bx0 = P.x0 & ~31, by0 = P.y0 & ~7;
  const int nbx = ((P.x1 | 31) - bx0 + 1) >> 5, nby = (((P.y1 | 7) - by0) >> 3) + 1;
  const int nblocks = nbx * nby;
  const int waves = (int)((gridDim.x * blockDim.x) >> 6);
  const int sx = P.lv.sx, sy = P.lv.sy;
  const unsigned int mtx = (unsigned int)mark_tiles_x(sx);
  auto marks_of = [&](int blk) -> unsigned int* {
    const int X0 = bx0 + ((blk % nbx) << 5), Y0 = by0 + ((blk / nbx) << 3);
    const unsigned int t0 = (((unsigned int)(Y0 >> 3) * mtx) + (unsigned int)(X0 >> 4)) << 7;  // byte index of the block's first tile
    return reinterpret_cast<unsigned int*>(P.lv.free_bytes + t0) + lane;
  };
  int blk = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  if (blk >= nblocks) return;
  unsigned int fw_next = *marks_of(blk);
  for (; blk < nblocks; blk += waves) {
    const unsigned int fw = fw_next;
    fw_next = blk + waves < nblocks ? *marks_of(blk + waves) : 0u;
    if (__ballot(fw != 0u) == 0ull) continue;  // wave-uniform: nothing of this scan in the block
    const int X0 = bx0 + ((blk % nbx) << 5), Y0 = by0 + ((blk / nbx) << 3);
    const int x = X0 + xl;
    if (fw != 0u) *marks_of(blk) = 0u;
    if (lane < 2) {
      const unsigned int t0 = (((unsigned int)(Y0 >> 3) * mtx) + (unsigned int)(X0 >> 4));
      P.lv.free_bytes[mark_tile_end_offset(sx, sy) + t0 + lane] = 0;
    }
    bool fre[4], occ[4];
    float l[4];
    unsigned int ko[4], kf[4];
    int st[4];  // STAMPED: the stored stamps
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 2 * i + rh, y = Y0 + r;
      const size_t c = (size_t)y * sx + x;
      // the byte of cell (xl, r): tile xl / 16, byte r * 16 + xl % 16 = dword (xl / 16) * 32 + r * 4 + (xl % 16) / 4, byte xl & 3
      const unsigned int fwd = (unsigned int)__shfl((int)fw, ((xl >> 4) << 5) + (r << 2) + ((xl & 15) >> 2));
      const unsigned int mark = (fwd >> ((xl & 3) << 3)) & 0xffu;
      occ[i] = (mark & kMarkEnd) != 0u && y < sy && x < sx;
      fre[i] = (mark & kMarkCrossed) != 0u && y < sy && x < sx;
      l[i] = 0.0f;
      ko[i] = kf[i] = 0u;
      st[i] = -1;
      if (fre[i] || occ[i]) l[i] = P.lv.logodds[c];
      if (STAMPED && (fre[i] || occ[i])) st[i] = P.lv.update_index[c];
      if (occ[i]) {
        ko[i] = P.lv.key_occ[c];
        kf[i] = P.lv.key_free[key_free_index(P.lv, (unsigned int)x, (unsigned int)y)];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int y = Y0 + 2 * i + rh;
      const size_t c = (size_t)y * sx + x;
      bool is_occ = occ[i], is_fre = fre[i];
      if (is_occ) {
        is_occ = (ko[i] >> kBeamBits) == P.serial;
        is_fre = (kf[i] >> kBeamBits) == P.serial;
      }
      if (!is_fre && !is_occ) continue;
      // the stored stamp (apply_box): at or past the occupied mark the cell stays; equal to the free mark it takes no free update
      const bool stored_free = STAMPED && st[i] == P.mark_free;
      if (STAMPED && (st[i] >= P.mark_occ || (stored_free && !is_occ))) continue;
      float lo = l[i];
      int stamp;
      if (is_occ) {
        // crossed by a beam of lower index than the first that ends here: applied, then reverted (:231-233).  Visible in the bits
        // only where lo + f leaves lo's binade (cells just above -2, -4, -8 ...): tests/test_gpu_update_order.py
        if (stored_free) {
          lo -= P.log_odds_free;
        } else if (is_fre && (kBeamMask - (kf[i] & kBeamMask)) < (kBeamMask - (ko[i] & kBeamMask))) {
          lo += P.log_odds_free;
          lo -= P.log_odds_free;
        }
        if (lo < 50.0f) lo += P.log_odds_occ;
        stamp = P.mark_occ;
      } else {
        lo += P.log_odds_free;
        stamp = P.mark_free;
      }
      __builtin_nontemporal_store(lo, &P.lv.logodds[c]);
      __builtin_nontemporal_store(stamp, &P.lv.update_index[c]);
      const float p = grid_probability(lo);
      __builtin_nontemporal_store(p, &P.lv.prob[c]);
      if (SCATTER_TEXELS) {
        float* q = reinterpret_cast<float*>(P.lv.quad);
        const bool lastx = x == sx - 1, lasty = y == sy - 1;
        auto put = [&](int tx, int ty, int comp) { q[4 * (size_t)quad_index(tx, ty, P.lv.tiles_x, sx) + comp] = p; };
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
    }
  }
}

// dense over the box grown by one cell towards -x/-y: texel (x,y) holds P of (x..x+1, y..y+1)
__global__ void __launch_bounds__(256) update_texels_kernel(const UpdateBatch B) {
  const UpdateParams& P = B.lv[blockIdx.y];
  if (P.x1 < P.x0) return;
  const int tx0 = P.x0 > 0 ? P.x0 - 1 : 0, ty0 = P.y0 > 0 ? P.y0 - 1 : 0;
  const int w = P.x1 - tx0 + 1, h = P.y1 - ty0 + 1;
  const size_t n = (size_t)w * h;
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
    const int x = tx0 + (int)(t % (size_t)w), y = ty0 + (int)(t / (size_t)w);
    const int xn = x + 1 < P.lv.sx ? x + 1 : x;
    const int yn = y + 1 < P.lv.sy ? y + 1 : y;
    const float* p = P.lv.prob;
    P.lv.quad[quad_index(x, y, P.lv.tiles_x, P.lv.sx)] =
        make_float4(p[(size_t)y * P.lv.sx + x], p[(size_t)y * P.lv.sx + xn], p[(size_t)yn * P.lv.sx + x],
                    p[(size_t)yn * P.lv.sx + xn]);
  }
}

// ---- posed scans that are already on the device (hsm_update_by_scans_device) ---------------------------------------------
// The host knows neither a scan's pose nor its length, so everything prepare_level() / level_bbox() derive from them on the
// host is derived here:
//   update_prep_kernel        one launch per call, one wavefront per scan (lane = level): scan k's UpdateBatch, in a
//                             context-owned device array, from d_poses_world[k] -- the fp32 expressions of prepare_level()
//   update_mark_scan_kernel   update_mark_kernel's two block kinds on that UpdateBatch, read through a pointer (wave-uniform
//                             address: scalar loads); the grid is sized by the caller's hint and strides over the scan's real
//                             beam count.  Its end-cell blocks also reduce the scan's cell box (DPP min / max per wavefront,
//                             one lane's atomicMin / atomicMax) into the scan's box, the level's running dirty box and its
//                             publish box (occupancy_kernels.h).  Cell boxes: map_cells.h.
//   update_apply_scan_kernel  apply_box() over that box, in a grid sized for the whole level (the host cannot size it by a
//                             box it never sees); a later launch on the same stream, so the box is complete.
// Keyed form for every scan length (correct for any length; the byte-map form needs per-beam records sized by the host).

struct UpdatePrepLevel {
  LevelRW lv;
  Affine2 mapTworld;
  float pt_scale;                 // 2^-level: DataContainer::setFrom (DataPointContainer.h:46-58)
  float origo_x, origo_y;         // the container's origo on this level (setFrom :48)
  float log_odds_free, log_odds_occ;
  unsigned int serial0;           // the level's key generation before the call: scan k takes ((serial0 + k) % kSerialMax) + 1
  int update_index0;              // currUpdateIndex before the call: scan k marks with update_index0 + 3 k + 1 / + 2
};

struct UpdatePrepParams {
  UpdatePrepLevel lv[kMaxLevels];
  int nlev, count;
  const float* poses_world;  // [count * 3]
  const float2* pts;
  const int* offsets;        // [count + 1] CSR offsets in points, or nullptr: every pose integrates pts[0 .. shared_n)
  int shared_n;
  const float2* origos;      // [count] the containers' origos in level-0 cell units, level l sees origos[k] * 2^-l (setFrom :48);
                             // or nullptr: the host pair UpdatePrepLevel::origo_x/y for every scan
  UpdateBatch* out;          // [count]
  int* boxes;                // [(count + 2) * kMaxLevels * 4]: slot 0 the running dirty boxes, slot 1 the LAST scan's, 2 + k scan k's
};

// the box slot of scan k of a call of `count` scans (the last scan's sits where the host finds it without knowing count)
__host__ __device__ __forceinline__ int update_box_slot(int k, int count) { return k == count - 1 ? 1 : 2 + k; }

// scan k's UpdateParams of level l and its (empty) box: points [first, first + n) of A.pts at `pose`, marked with
// update_index0 + 3 * rank + 1 / + 2 (currMarkFreeIndex / currMarkOccIndex, OccGridMapBase.h:123-124).  `origo`: with
// A.origos, the level-0 origo of the container this level integrates (the scan's own, or the retained scan's on the coarse
// levels of a forced scan); not read otherwise.
__device__ __forceinline__ void update_prep_scan_level(const UpdatePrepParams& A, int k, int l, float px, float py, float th,
                                                       int first, int n, int rank, float2 origo) {
  const UpdatePrepLevel& V = A.lv[l];
  UpdateParams P;
  P.lv = V.lv;
  float mx, my;
  affine_apply(V.mapTworld, px, py, mx, my);  // getMapCoordsPose
  // Translation2f(mapPose.xy) * Rotation2Df(mapPose.theta): glibc's sinf / cosf (the pair sincosf returns, libm_exact.h)
  float sinA, cosA;
  libm::sincosf_glibc<false>(th, sinA, cosA);
  P.pose.l00 = cosA;
  P.pose.l01 = -sinA;
  P.pose.l10 = sinA;
  P.pose.l11 = cosA;
  P.pose.t0 = mx;
  P.pose.t1 = my;
  // setFrom's origo * factor (DataPointContainer.h:48): one fp32 multiply per component, level 0 takes the origo as it is --
  // the expression the host evaluates for the pair it passes
  const float ox = A.origos == nullptr ? V.origo_x : (l == 0 ? origo.x : origo.x * V.pt_scale);
  const float oy = A.origos == nullptr ? V.origo_y : (l == 0 ? origo.y : origo.y * V.pt_scale);
  float bx, by;
  affine_apply(P.pose, ox, oy, bx, by);
  bx += 0.5f;
  by += 0.5f;
  // x86's truncating conversion makes a NaN or out-of-range begin coordinate INT_MIN, which fails the map test of every beam;
  // this device's makes a NaN 0, a VALID cell.  beam_line()'s finite-range test, applied to the begin cell: what it rejects is
  // outside the map in the reference too, and (-1, -1) drops every beam the same way.
  const bool finite = bx > -2.0f && bx < (float)V.lv.sx + 2.0f && by > -2.0f && by < (float)V.lv.sy + 2.0f;
  P.bx = finite ? (int)bx : -1;
  P.by = finite ? (int)by : -1;
  if (n < 0 || n > (int)kBeamMask) n = 0;  // (more beams than the key's index field holds: integrated as an empty scan)
  P.pts = A.pts + first;
  P.n = n;
  P.pt_scale = V.pt_scale;
  P.serial = (V.serial0 + (unsigned int)k) % kSerialMax + 1u;
  P.log_odds_free = V.log_odds_free;
  P.log_odds_occ = V.log_odds_occ;
  P.mark_free = V.update_index0 + 3 * rank + 1;
  P.mark_occ = V.update_index0 + 3 * rank + 2;
  P.x0 = P.y0 = kBoxEmptyLo;  // (the passes take the box from A.boxes)
  P.x1 = P.y1 = kBoxEmptyHi;
  P.recs = nullptr;
  UpdateBatch& B = A.out[k];
  B.lv[l] = P;
  if (l == 0) B.nlev = A.nlev;
  int* box = A.boxes + ((size_t)update_box_slot(k, A.count) * kMaxLevels + l) * 4;
  box[0] = box[1] = kBoxEmptyLo;
  box[2] = box[3] = kBoxEmptyHi;
}

__global__ void __launch_bounds__(64) update_prep_kernel(const UpdatePrepParams A) {
  const int k = blockIdx.x, l = threadIdx.x;
  if (l >= A.nlev) return;
  int first = 0, n = A.shared_n;
  if (A.offsets) {
    first = A.offsets[k];
    n = A.offsets[k + 1] - first;
  }
  // every scan is integrated: scan k is update k of the call
  const float2 origo = A.origos ? A.origos[k] : make_float2(0.0f, 0.0f);
  update_prep_scan_level(A, k, l, A.poses_world[3 * k], A.poses_world[3 * k + 1], A.poses_world[3 * k + 2], first, n, k, origo);
}

// ---- the movement gate in front of them (hsm_update_by_scans_device_gated, hsm_slam_scans_device) -------------------------------
// HectorSlamProcessor::update (HectorSlamProcessor.h:71-95) integrates a scan only where util::poseDifferenceLargerThan(pose,
// lastMapUpdatePose, ..) holds or the caller forces it, and lastMapUpdatePose follows every integrated scan: the decisions of a
// call are SEQUENTIAL in k, and the host sees none of them.  So what the host derived per scan for the ungated entry -- "scan k is
// update k" -- is derived here: ONE launch per call, one workgroup.  Lane 0 walks the scans, 256 a turn (update_gate.h's
// gate_step, the text the CPU model test compiles), and leaves {integrated, rank, the coarse levels' points} per scan in LDS;
// then all lanes fill the UpdateBatch blocks as update_prep_kernel does.  A rejected scan gets n = 0 on every level and an empty
// box: update_mark_scan_kernel and update_apply_scan_kernel return after one scalar load.  The gate's state lives in a
// per-context device block and is written with ordinary stores.
struct GateState {
  float last_update_pose[3];  // lastMapUpdatePose: FLT_MAX three times until a scan is integrated
  int pending;                // updates that gated calls applied and the host has not yet folded into Level's counters
  // hsm_slam_scans_device
  float hint[3];              // start estimate of the next scan
  int retained_first;         // the scan the coarse levels retain (matchData's setFrom, MapRepMultiMap.h:143): points
  float last_pose[3];         // lastScanMatchPose                                   [retained_first, + retained_n) of this
  int retained_n;             //                                                     call's d_pts_xy
  float last_cov[9];          // lastScanMatchCov
  float retained_origo[2];    // the retained scan's origo, level-0 cell units (setFrom copies it with the points, :48); read
  int reserved[1];            // only by calls that carry per-scan origos
};
static_assert(sizeof(GateState) == 24 * 4, "GateState: six 16-byte rows");

struct UpdateGateParams {
  UpdatePrepParams prep;
  GateState* state;
  float min_dist, min_angle;
  const unsigned char* force;  // [count] map_without_matching per scan, or nullptr
  int* out_applied;            // [count], or nullptr
  // hsm_slam_scans_device's call for ONE scan (count == 1), behind its match:
  int slam;
  float* pose_io;              // [3] the matched pose; a forced scan takes its hint instead (written here)
  float* cov_io;               // [9] the match's covariance, or nullptr; a forced scan keeps the last one (written here)
  const float* next_delta;     // [3] added to the pose to give the next scan's hint, or nullptr: the pose itself
};

constexpr int kGateChunk = 256;

__global__ void __launch_bounds__(256) update_gate_prep_kernel(const UpdateGateParams G) {
  __shared__ int4 walk[kGateChunk];  // {integrated, rank, first point of the coarse levels' container, its length}
  __shared__ float2 walk_origo[kGateChunk];  // that container's origo (per-scan origos only)
  const UpdatePrepParams& A = G.prep;
  GateWalk w;
  gate_reset(w);
  GateRetained ret;
  gate_retained_reset(ret);
  if (threadIdx.x == 0) {
    w.last_update_pose[0] = G.state->last_update_pose[0];
    w.last_update_pose[1] = G.state->last_update_pose[1];
    w.last_update_pose[2] = G.state->last_update_pose[2];
    w.applied = G.state->pending;
    ret.first = G.state->retained_first;
    ret.n = G.state->retained_n;
    ret.origo[0] = G.state->retained_origo[0];
    ret.origo[1] = G.state->retained_origo[1];
  }
  for (int k0 = 0; k0 < A.count; k0 += kGateChunk) {
    const int chunk = min(kGateChunk, A.count - k0);
    if (threadIdx.x == 0) {
      for (int j = 0; j < chunk; ++j) {
        const int k = k0 + j;
        const bool force = G.force != nullptr && G.force[k] != 0;
        int first = 0, n = A.shared_n;
        if (A.offsets) {
          first = A.offsets[k];
          n = A.offsets[k + 1] - first;
        }
        const float2 own = A.origos ? A.origos[k] : make_float2(0.0f, 0.0f);
        float pose[3];
        if (G.slam) {
          // a forced scan skips the match (HectorSlamProcessor.h:75-80): its pose is its hint, the covariance stays, and the
          // coarse levels keep the containers of the last matched scan
          for (int i = 0; i < 3; ++i) pose[i] = force ? G.state->hint[i] : G.pose_io[3 * k + i];
          if (force)
            for (int i = 0; i < 3; ++i) G.pose_io[3 * k + i] = pose[i];
          gate_retain_step(ret, force, first, n, own.x, own.y);
          if (G.cov_io) {
            for (int i = 0; i < 9; ++i) {
              if (force)
                G.cov_io[9 * k + i] = G.state->last_cov[i];
              else if (n > 0)  // (matchData leaves the covariance alone for an empty container, ScanMatcher.h:62-64)
                G.state->last_cov[i] = G.cov_io[9 * k + i];
            }
          }
          for (int i = 0; i < 3; ++i) {
            G.state->last_pose[i] = pose[i];
            G.state->hint[i] = G.next_delta ? pose[i] + G.next_delta[i] : pose[i];
          }
        } else {
          for (int i = 0; i < 3; ++i) pose[i] = A.poses_world[3 * k + i];
          gate_retain_step(ret, false, first, n, own.x, own.y);  // every level sees the scan itself, as in hsm_update_by_scans_device
        }
        int rank;
        const bool go = gate_step(w, pose, force, G.min_dist, G.min_angle, &rank);
        walk[j] = make_int4(go ? 1 : 0, rank, ret.first, ret.n);
        walk_origo[j] = make_float2(ret.origo[0], ret.origo[1]);
        if (G.out_applied) G.out_applied[k] = go ? 1 : 0;
      }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < chunk * A.nlev; t += blockDim.x) {
      const int j = t / A.nlev, l = t - j * A.nlev, k = k0 + j;
      const int4 d = walk[j];
      int first = 0, n = A.shared_n;
      if (A.offsets) {
        first = A.offsets[k];
        n = A.offsets[k + 1] - first;
      }
      float2 origo = A.origos ? A.origos[k] : make_float2(0.0f, 0.0f);
      if (l > 0) {
        first = d.z;
        n = d.w;
        origo = walk_origo[j];
      }
      const float* pose = G.slam ? G.pose_io + 3 * k : A.poses_world + 3 * k;
      update_prep_scan_level(A, k, l, pose[0], pose[1], pose[2], first, d.x ? n : 0, d.y, origo);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    G.state->last_update_pose[0] = w.last_update_pose[0];
    G.state->last_update_pose[1] = w.last_update_pose[1];
    G.state->last_update_pose[2] = w.last_update_pose[2];
    G.state->pending = w.applied;
    G.state->retained_first = ret.first;
    G.state->retained_n = ret.n;
    G.state->retained_origo[0] = ret.origo[0];
    G.state->retained_origo[1] = ret.origo[1];
  }
}

// lastMapUpdatePose back to FLT_MAX (hsm_reset_update_gate); `all`: lastScanMatchPose and the hint back to 0 as well
// (HectorSlamProcessor::reset, HectorSlamProcessor.h:133-140).  The counters stay: the maps keep theirs.
__global__ void update_gate_reset_kernel(GateState* state) {
  if (threadIdx.x < 3) {
    state->last_update_pose[threadIdx.x] = FLT_MAX;
    state->last_pose[threadIdx.x] = 0.0f;
    state->hint[threadIdx.x] = 0.0f;
  }
}

// hsm_slam_scans_device, in front of the first scan of a call: its hint is the start pose -- or, where the caller gives none,
// the last pose of the call before -- plus delta 0; the coarse levels' containers do not outlive the call that owned their points
__global__ void slam_begin_kernel(GateState* state, const float* __restrict__ start_pose, const float* __restrict__ delta0) {
  if (threadIdx.x < 3) {
    const float p = start_pose ? start_pose[threadIdx.x] : state->last_pose[threadIdx.x];
    state->hint[threadIdx.x] = delta0 ? p + delta0[threadIdx.x] : p;
  }
  if (threadIdx.x == 0) {
    state->retained_first = 0;
    state->retained_n = 0;
    state->retained_origo[0] = state->retained_origo[1] = 0.0f;
  }
}

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}
// min / max over the wavefront, in every lane (all 64 lanes active): the 16-lane rows by DPP, the four rows by readlane
__device__ __forceinline__ int wave_min_i32(int v) {
  v = min(v, dpp_i32<0xB1>(v));   // quad_perm [1,0,3,2]
  v = min(v, dpp_i32<0x4E>(v));   // quad_perm [2,3,0,1]
  v = min(v, dpp_i32<0x141>(v));  // row_half_mirror
  v = min(v, dpp_i32<0x140>(v));  // row_mirror
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ int wave_max_i32(int v) {
  v = max(v, dpp_i32<0xB1>(v));
  v = max(v, dpp_i32<0x4E>(v));
  v = max(v, dpp_i32<0x141>(v));
  v = max(v, dpp_i32<0x140>(v));
  return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// The cell box of everything beams [block * 256, block * 256 + 256) of the scan can touch: the hull of the end cells of its
// non-skipped beams and the begin cell (a Bresenham line stays inside the box of its end points) -- every cell a mark pass
// writes to, so the apply pass over it clears every mark.  level_bbox() on the host also counts beams that end IN the begin
// cell (skipped, OccGridMapBase.h:158): its box is this one, or the begin cell alone where this one is empty.
// Called by all 64 lanes of every wavefront.
__device__ __forceinline__ void mark_box_block(const UpdateParams& P, unsigned int block, int* scan_box, int* run_box,
                                               int* pub_box) {
  const int beam = block * blockDim.x + threadIdx.x;
  int x0 = kBoxEmptyLo, y0 = kBoxEmptyLo, x1 = kBoxEmptyHi, y1 = kBoxEmptyHi;
  if (beam < P.n) {
    const BeamLine b = beam_line(P, beam);
    if (b.valid) {
      x0 = x1 = b.x1;
      y0 = y1 = b.y1;
    }
  }
  x1 = wave_max_i32(x1);
  if (x1 < 0) return;  // wave-uniform: no beam of this wavefront ends inside the map
  x0 = min(wave_min_i32(x0), P.bx);
  y0 = min(wave_min_i32(y0), P.by);
  x1 = max(x1, P.bx);
  y1 = max(wave_max_i32(y1), P.by);
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&scan_box[0], x0);
    atomicMin(&scan_box[1], y0);
    atomicMax(&scan_box[2], x1);
    atomicMax(&scan_box[3], y1);
    atomicMin(&run_box[0], x0);
    atomicMin(&run_box[1], y0);
    atomicMax(&run_box[2], x1);
    atomicMax(&run_box[3], y1);
    atomicMin(&pub_box[0], x0);
    atomicMin(&pub_box[1], y0);
    atomicMax(&pub_box[2], x1);
    atomicMax(&pub_box[3], y1);
  }
}

// gridDim.x = occ_blocks + free_blocks, sized by the caller's hint: the first occ_blocks workgroups of a row mark end cells and
// reduce the box, 256 beams a turn, the others walk lines, 4 beams a turn, until the scan's real beam count is covered
__global__ void __launch_bounds__(256) update_mark_scan_kernel(const UpdateBatch* __restrict__ B, unsigned int occ_blocks,
                                                               int* scan_boxes, int* run_boxes, int* pub_boxes) {
  const UpdateParams P = B->lv[blockIdx.y];
  if (P.n <= 0) return;
  if (blockIdx.x < occ_blocks) {
    const unsigned int turns = ((unsigned int)P.n + 255u) / 256u;
    for (unsigned int b = blockIdx.x; b < turns; b += occ_blocks) {
      mark_occ_block(P, b);
      mark_box_block(P, b, scan_boxes + 4 * blockIdx.y, run_boxes + 4 * blockIdx.y, pub_boxes + 4 * blockIdx.y);
    }
  } else {
    const unsigned int free_blocks = gridDim.x - occ_blocks, turns = ((unsigned int)P.n + 3u) / 4u;
    for (unsigned int b = blockIdx.x - occ_blocks; b < turns; b += free_blocks) mark_free_block(P, b);
  }
}

template <bool SCATTER_TEXELS, bool STAMPED>
__global__ void __launch_bounds__(256) update_apply_scan_kernel(const UpdateBatch* __restrict__ B,
                                                                const int* __restrict__ scan_boxes) {
  const int4 box = *reinterpret_cast<const int4*>(scan_boxes + 4 * blockIdx.y);
  if (box.z < box.x) return;  // nothing of this scan on this level
  UpdateParams P = B->lv[blockIdx.y];
  P.x0 = box.x;
  P.y0 = box.y;
  P.x1 = box.z;
  P.y1 = box.w;
  apply_box<SCATTER_TEXELS, STAMPED>(P, blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// the running dirty boxes of all levels back to empty (after the host has merged them)
__global__ void update_boxes_clear_kernel(int* boxes, int n_boxes) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * n_boxes) boxes[i] = (i & 3) < 2 ? kBoxEmptyLo : kBoxEmptyHi;
}

// ---- whole-plane maintenance (create / reset / upload) ------------------------------
__global__ void fill_level_kernel(LevelRW L, float logodds, int update_index) {
  const size_t n = (size_t)L.sx * L.sy;
  const float p = grid_probability(logodds);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    L.logodds[i] = logodds;
    L.update_index[i] = update_index;
    L.prob[i] = p;
  }
  // every texel of the tiled plane, including the padding of partial edge tiles
  if (L.quad) {  // the plane layout keeps no texel plane
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)L.quad_texels;
         i += (size_t)gridDim.x * blockDim.x) {
      L.quad[i] = make_float4(p, p, p, p);
    }
  }
}

__global__ void rebuild_prob_kernel(LevelRW L) {
  const size_t n = (size_t)L.sx * L.sy;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    L.prob[i] = grid_probability(L.logodds[i]);
  }
}

// texel (x,y) from the probability plane; the last row/column (never sampled: the
// bounds test keeps ix,iy <= size-2) replicate the edge
__global__ void rebuild_quad_kernel(LevelRW L) {
  const size_t n = (size_t)L.sx * L.sy;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % (size_t)L.sx), y = (int)(i / (size_t)L.sx);
    const int x1 = x + 1 < L.sx ? x + 1 : x;
    const int y1 = y + 1 < L.sy ? y + 1 : y;
    L.quad[quad_index(x, y, L.tiles_x, L.sx)] = make_float4(L.prob[(size_t)y * L.sx + x], L.prob[(size_t)y * L.sx + x1],
                            L.prob[(size_t)y1 * L.sx + x], L.prob[(size_t)y1 * L.sx + x1]);
  }
}

}  // namespace hsm
