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
// Here: host-posed updates, plane maintenance.  update_types.h: shared with map_update_scans.h; update_cell_rule.h: the cell rule.
#pragma once
#include "update_types.h"

namespace hsm {

// passes 1a + 1b of a SMALL scan in one launch: the first occ_blocks workgroups of a row mark the end cells, the rest
// walk the lines with keyed atomics (no dependency between the two, see mark_free_block)
__global__ void __launch_bounds__(256) update_mark_kernel(const UpdateBatch B, unsigned int occ_blocks) {
  const UpdateParams& P = B.lv[blockIdx.y];
  if (blockIdx.x < occ_blocks)
    mark_occ_block(P, blockIdx.x);
  else
    mark_free_block(P, blockIdx.x - occ_blocks);
}

template <bool SCATTER_TEXELS, bool STAMPED>
__global__ void __launch_bounds__(256) update_apply_kernel(const UpdateBatch B) {
  apply_box<SCATTER_TEXELS, STAMPED>(B.lv[blockIdx.y], blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x);
}

// pass 1a of a dense scan: the occ key as mark_occ_block writes it; the end-cell flag goes into the cell's MARK BYTE (value 2)
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
      const CellUpdate u = update_cell_rule<STAMPED>(l[i], st[i], is_occ, is_fre, kBeamMask - (ko[i] & kBeamMask),
                                                     kBeamMask - (kf[i] & kBeamMask), P.log_odds_free, P.log_odds_occ, P.mark_free, P.mark_occ);
      if (!u.written) continue;
      __builtin_nontemporal_store(u.logodds, &P.lv.logodds[c]);
      __builtin_nontemporal_store(u.stamp, &P.lv.update_index[c]);
      const float p = grid_probability(u.logodds);
      __builtin_nontemporal_store(p, &P.lv.prob[c]);
      if (SCATTER_TEXELS) scatter_texels(P.lv, x, y, p);
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
