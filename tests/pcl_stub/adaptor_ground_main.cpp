// TEST INFRASTRUCTURE: drives mi355ndt::NormalDistributionsTransformGround of include/mi355_ndt_pcl.hpp the way lv_slam's odometry nodelet
// configures its ground_s2k object (scan_matching_odom_nodelet.cpp:121-126, 329), against tests/pcl_stub's stand-in for pcl::Registration.
//   adaptor_ground_main <target.f32> <source.f32> <n_target> <n_source> <resolution>
// clouds are raw float32 x,y,z triples; prints one line: final 16, last increment 16, iterations, converged, trans_probability, the engine's
// MI355NDT_OPT_GROUND_CLASS, the code setGroundClass(7) returns.
#include <cstdio>
#include <cstdlib>
#include "mi355_ndt_pcl.hpp"

typedef pcl::PointXYZI PointT;

static pcl::PointCloud<PointT>::Ptr load(const char* path, size_t n) {
  pcl::PointCloud<PointT>::Ptr c(new pcl::PointCloud<PointT>());
  c->points.resize(n);
  FILE* f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  for (size_t i = 0; i < n; i++) {
    float v[3];
    if (fread(v, sizeof(float), 3, f) != 3) { fprintf(stderr, "short read\n"); exit(2); }
    c->points[i].x = v[0]; c->points[i].y = v[1]; c->points[i].z = v[2]; c->points[i].data[3] = 1.f; c->points[i].intensity = 0.f;
  }
  fclose(f);
  c->width = (unsigned)n;
  return c;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const size_t nt = strtoul(argv[3], 0, 10), ns = strtoul(argv[4], 0, 10);
  pcl::PointCloud<PointT>::Ptr tgt = load(argv[1], nt), src = load(argv[2], ns);
  mi355ndt::NormalDistributionsTransformGround<PointT, PointT> ground_s2k;        // scan_matching_odom_nodelet.cpp:329
  // :121-126
  ground_s2k.setNumThreads(4);
  ground_s2k.setTransformationEpsilon(0.01);
  ground_s2k.setMaximumIterations(64);
  ground_s2k.setResolution((float)atof(argv[5]));
  ground_s2k.setNeighborhoodSearchMethod(mi355ndt::DIRECT1);
  ground_s2k.setInputTarget(tgt);
  ground_s2k.setInputSource(src);
  Eigen::Matrix4f guess = Eigen::Matrix4f::Identity();
  guess(0, 3) = 1.0f;
  pcl::PointCloud<PointT> out;
  ground_s2k.align(out, guess);
  const Eigen::Matrix4f F = ground_s2k.getFinalTransformation(), L = ground_s2k.getLastIncrementalTransformation();
  for (int i = 0; i < 16; i++) printf("%.9g ", F.data()[i]);
  for (int i = 0; i < 16; i++) printf("%.9g ", L.data()[i]);
  int cls = -1;
  mi355ndt_get_option(ground_s2k.handle(), MI355NDT_OPT_GROUND_CLASS, &cls);
  const int bad = ground_s2k.setGroundClass(7);
  printf("%d %d %.17g %d %d\n", ground_s2k.getFinalNumIteration(), (int)ground_s2k.hasConverged(), ground_s2k.getTransformationProbability(), cls, bad);
  return 0;
}
