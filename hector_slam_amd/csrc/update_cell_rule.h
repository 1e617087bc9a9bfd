// update_cell_rule.h -- what one scan does to one cell: bresenhamCellFree / bresenhamCellOcc (HSL/map/OccGridMapBase.h:216-241)
// over the cell rules of GridMapLogOdds.h:135-156, as the net effect per scan and cell that map_update.h's header derives.
// Plain C++ (no HIP header, nothing else of csrc/): both apply passes and tests/cpp/update_cell_rule_check.cpp compile this text.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HSM_RULE_HD __host__ __device__ __forceinline__
#else
#define HSM_RULE_HD inline
#endif

namespace hsm {

struct CellUpdate { bool written; float logodds; int stamp; };  // not written: log-odds, stamp, probability and texels stay

// l, s: the cell's log-odds and its stored stamp; s is read only when STAMPED (restored levels, map_update.h "Stored stamps":
// the reference's tests on the stamp are applied).  occ / fre: a beam of this scan ends here / crosses here; beam_occ / beam_fre:
// the lowest index of such a beam (compared only where both hold).  f, o: the level's free and occupied log-odds steps.
template <bool STAMPED>
HSM_RULE_HD CellUpdate update_cell_rule(float l, int s, bool occ, bool fre, unsigned int beam_occ, unsigned int beam_fre,
                                        float f, float o, int mark_free, int mark_occ) {
  const CellUpdate untouched = {false, 0.0f, 0};
  if (!fre && !occ) return untouched;
  bool stored_free = false;  // the stored stamp IS this scan's free mark: no free update, unsetFree in front of the occupied one
  if (STAMPED) {
    if (s >= mark_occ) return untouched;  // :228 fails, and :218 with it: the cell stays as it is
    stored_free = s == mark_free;
    if (stored_free && !occ) return untouched;  // :218 fails
  }
  int stamp;
  if (occ) {
    // free-touched by an earlier beam of this scan: applied, then reverted (:231-233)
    // (in fp32 (l + f) - f == l unless l + f leaves l's binade, so this comparison shows in the bits only for cells just above
    // -2, -4, -8 ...: tests/test_gpu_update_order.py puts cells there and runs scans in several beam orders)
    if (stored_free) {
      l -= f;
    } else if (fre && beam_fre < beam_occ) {
      l += f;
      l -= f;
    }
    if (l < 50.0f) l += o;  // updateSetOccupied
    stamp = mark_occ;
  } else {
    l += f;                // updateSetFree
    stamp = mark_free;
  }
  return {true, l, stamp};
}

}  // namespace hsm
