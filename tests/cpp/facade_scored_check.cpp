// Compile check of the facade's scored batch entry (tests/test_score_batch_abi.py): instantiates
// MapRepMultiMap::matchDataBatchScored with the types a caller passes.  Never run.
#include <vector>

#include "slam_main/HectorSlamProcessor.h"  // pulls the facade in behind what it needs, as the node does

int facade_scored_check(hectorslam::MapRepMultiMap& rep, const hectorslam::DataContainer& scan) {
  std::vector<Eigen::Vector3f> begin(64, Eigen::Vector3f(0.0f, 0.0f, 0.0f)), poses;
  std::vector<const hectorslam::DataContainer*> scans(begin.size(), &scan);
  std::vector<float> likelihoods;
  std::vector<Eigen::Matrix3f> cov;
  std::vector<int> best;
  rep.matchDataBatchScored(begin, scans, poses, likelihoods);
  rep.matchDataBatchScored(begin, scans, poses, likelihoods, &cov, 0, 32, &best);
  rep.matchDataBatch(begin, scans, poses, &cov);
  return static_cast<int>(best.size() + likelihoods.size());
}
