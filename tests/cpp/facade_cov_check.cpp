// Compile check of the facade's batched covariance entry (tests/test_covariance_batch_abi.py): instantiates
// MapRepMultiMap::getCovarianceForPosesBatch with the types a caller passes.  Never run.
#include <vector>

#include "slam_main/HectorSlamProcessor.h"  // pulls the facade in behind what it needs, as the node does

int facade_cov_check(hectorslam::MapRepMultiMap& rep, const hectorslam::DataContainer& scan) {
  std::vector<Eigen::Vector3f> poses(64, Eigen::Vector3f(0.0f, 0.0f, 0.0f));
  std::vector<const hectorslam::DataContainer*> scans(poses.size(), &scan);
  std::vector<Eigen::Matrix3f> cov;
  std::vector<float> likelihoods;
  rep.getCovarianceForPosesBatch(poses, scans, cov);
  rep.getCovarianceForPosesBatch(poses, scans, cov, &likelihoods, 1);
  return static_cast<int>(cov.size() + likelihoods.size());
}
