// update_gate.h -- the movement gate of HectorSlamProcessor::update (HSL/slam_main/HectorSlamProcessor.h:71-95): a scan is
// integrated into the map only when its pose differs from the pose of the last integrated scan by more than a distance or an
// angle, util::poseDifferenceLargerThan (HSL/util/UtilFunctions.h:73-92), or when the caller forces it (map_without_matching).
// Plain C++ (no HIP header): the device's gate kernel (map_update_scans.h) and the host compile the same text, and
// tests/cpp/update_gate_model.cpp holds it to the CPU checkers with the host compiler alone (tests/test_update_gate_model.py).
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HSM_GATE_HD __host__ __device__
#else
#define HSM_GATE_HD
#endif

namespace hsm {

// HectorSlamProcessor.h:62-63
constexpr float kGateDefaultMinDist = 0.4f, kGateDefaultMinAngle = 0.13f;

// util::poseDifferenceLargerThan in the reference's own mix of types:
//   ((pose1.head<2>() - pose2.head<2>()).norm()) > distanceDiffThresh     fp32: sqrtf(dx * dx + dy * dy), the products and the sum
//                                                                          each rounded (no contraction), the root correctly rounded
//   angleDiff > M_PI / < -M_PI                                             the float against the DOUBLE constant
//   angleDiff -= M_PI * 2.0f  /  += M_PI * 2.0f                            in double, rounded back to float
//   abs(angleDiff) > angleDiffThresh                                       fp32
// A NaN in any component compares false everywhere: "not larger".  Against (FLT_MAX, FLT_MAX, .) the squared distance
// overflows to +inf: "larger".
HSM_GATE_HD inline bool pose_difference_larger_than(const float pose1[3], const float pose2[3], float dist_thresh,
                                                    float angle_thresh) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float dx = pose1[0] - pose2[0];
  const float dy = pose1[1] - pose2[1];
  const float xx = dx * dx, yy = dy * dy;
  const float sq = xx + yy;
  if (sqrtf(sq) > dist_thresh) return true;
  float angle_diff = pose1[2] - pose2[2];
  const double pi = 3.14159265358979323846;  // M_PI
  if ((double)angle_diff > pi) {
    angle_diff = (float)((double)angle_diff - pi * 2.0);
  } else if ((double)angle_diff < -pi) {
    angle_diff = (float)((double)angle_diff + pi * 2.0);
  }
  return fabsf(angle_diff) > angle_thresh;
}

// What the gate remembers between scans: lastMapUpdatePose, FLT_MAX three times until the first scan is integrated
// (HectorSlamProcessor.h:133-136 reset()), and how many scans it has let through.
struct GateWalk {
  float last_update_pose[3];
  int applied;
};

HSM_GATE_HD inline void gate_reset(GateWalk& g) {
  g.last_update_pose[0] = g.last_update_pose[1] = g.last_update_pose[2] = FLT_MAX;
  g.applied = 0;
}

// One scan of HectorSlamProcessor::update's second half (:84-94): true = integrate it.  *rank = the number of scans integrated
// before it since `g.applied` was last zeroed, which numbers its update (OccGridMapBase.h:123-124, :167).  A rejected scan
// changes nothing.
HSM_GATE_HD inline bool gate_step(GateWalk& g, const float pose[3], bool map_without_matching, float dist_thresh,
                                  float angle_thresh, int* rank) {
  *rank = g.applied;
  if (!(pose_difference_larger_than(pose, g.last_update_pose, dist_thresh, angle_thresh) || map_without_matching)) return false;
  g.last_update_pose[0] = pose[0];
  g.last_update_pose[1] = pose[1];
  g.last_update_pose[2] = pose[2];
  ++g.applied;
  return true;
}

// What the coarse levels integrate (MapRepMultiMap.h:127,143): level 0 takes the scan's own container, level l >= 1 takes
// dataContainers[l-1], the copy matchData's setFrom made of the last MATCHED scan -- its points AND its origo
// (DataPointContainer.h:46-58).  Points [first, first + n) of the call's end points; origo in level-0 cell units, scaled by
// 2^-l where a level uses it.  n == 0 until a scan of the call has been matched.
struct GateRetained {
  int first, n;
  float origo[2];
};

HSM_GATE_HD inline void gate_retained_reset(GateRetained& r) {
  r.first = r.n = 0;
  r.origo[0] = r.origo[1] = 0.0f;
}

// One scan of HectorSlamProcessor::update's first half (:75-80) as the coarse levels see it: a scan that is matched (an empty
// one too: setFrom runs before the matcher looks at the size) replaces the retained container, whether or not the gate lets it
// through afterwards; a forced scan (`keeps`: the SLAM loop's map_without_matching) skips matchData and leaves it alone.
// Where no matcher runs (the gated update at given poses) every scan replaces it: every level sees the scan itself.
HSM_GATE_HD inline void gate_retain_step(GateRetained& r, bool keeps, int first, int n, float origo_x, float origo_y) {
  if (keeps) return;
  r.first = first;
  r.n = n;
  r.origo[0] = origo_x;
  r.origo[1] = origo_y;
}

}  // namespace hsm
