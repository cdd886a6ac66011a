// adapter.hpp -- header-only C++ host side above the C-ABI (badger_pf.h), shaped like the
// reference's classes so that Node2D-style code needs a type swap only:
//
//   badger_amcl_amd::OccupancyMap      <- OccupancyMap      (include/amcl/map/occupancy_map.h:54-123)
//   badger_amcl_amd::PlanarData        <- PlanarData        (include/amcl/sensors/planar_scanner.h:45-54)
//   badger_amcl_amd::PlanarScanner     <- PlanarScanner     (include/amcl/sensors/planar_scanner.h:57-168)
//   badger_amcl_amd::ParticleFilter    <- ParticleFilter    (include/amcl/pf/particle_filter.h:92-184)
//   badger_amcl_amd::PFSample / PFSampleSet                 (include/amcl/pf/particle_filter.h:41-87)
//   badger_amcl_amd::OdomData / Odom   <- OdomData / Odom   (include/amcl/sensors/odom.h:43-90)
//   badger_amcl_amd::OctoMap           <- OctoMap           (include/amcl/map/octomap.h:96-110, the LUT state)
//   badger_amcl_amd::PointCloudData    <- PointCloudData    (include/amcl/sensors/point_cloud_scanner.h:45-51)
//   badger_amcl_amd::PointCloudScanner <- PointCloudScanner (include/amcl/sensors/point_cloud_scanner.h:53-120)
//   badger_amcl_amd::ShardedParticleFilter       one rank of a filter sharded over several engines (one process each)
//   badger_amcl_amd::LocalShardedParticleFilter  all ranks of it in this process (bpf_shard_connect_local)
//
// Same method names, argument meaning and return conventions (false / 0.0 on the reference's
// silent failures); conditions the reference asserts on or hangs in surface as std::runtime_error.
// No Eigen / ROS / PCL dependency: poses are plain double[3].
#pragma once
#include <array>
#include <condition_variable>
#include <cstdint>
#include <cmath>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../badger_pf.h"

namespace badger_amcl_amd
{

enum MapCellState { CELL_FREE = -1, CELL_UNKNOWN = 0, CELL_OCCUPIED = 1 };
enum PFResampleModelType { PF_RESAMPLE_MULTINOMIAL = BPF_RESAMPLE_MULTINOMIAL, PF_RESAMPLE_SYSTEMATIC = BPF_RESAMPLE_SYSTEMATIC };

class Engine
{
public:
  explicit Engine(int device = 0)
  {
    const int rc = bpf_create(device, &h_);
    if (rc != BPF_OK)
      throw std::runtime_error(std::string("bpf_create: ") + bpf_error_string(rc));
  }
  ~Engine() { bpf_destroy(h_); }
  Engine(const Engine&) = delete;
  Engine& operator=(const Engine&) = delete;
  bpf_engine* get() const { return h_; }
  void check(int rc) const
  {
    if (rc != BPF_OK)
      throw std::runtime_error(std::string("bpf: ") + bpf_last_error_message(h_) + " (" + bpf_error_string(rc) + ")");
  }

private:
  bpf_engine* h_ = nullptr;
};

struct PFSample
{
  std::array<double, 3> pose;  // x, y, theta
  double weight;
};

// Pins a sample buffer the caller owns for as long as this object lives (bpf_host_buffer_register /
// _unregister): what a ParticleFilter that keeps its `samples` vector in host memory (allocated once at max_samples,
// particle_filter.cpp:62-89) holds beside the vector, so that applyModelToSampleSet / initWithSamples / getCurrentSet
// move it at PCIe rate.  The vector must not be resized while it is pinned.
class PinnedSamples
{
public:
  PinnedSamples(std::shared_ptr<Engine> e, std::vector<PFSample>& samples) : e_(std::move(e)), ptr_(samples.data())
  {
    e_->check(bpf_host_buffer_register(e_->get(), ptr_, samples.size() * sizeof(PFSample)));
  }
  ~PinnedSamples() { (void)bpf_host_buffer_unregister(e_->get(), ptr_); }
  PinnedSamples(const PinnedSamples&) = delete;
  PinnedSamples& operator=(const PinnedSamples&) = delete;

private:
  std::shared_ptr<Engine> e_;
  void* ptr_;
};
static_assert(sizeof(PFSample) == 32, "PFSample must match the reference's 32-byte AoS record");

// One Gaussian component of a mixture initialiser (ParticleFilter::initWithMixture): bpf_mixture_component as it is
using MixtureComponent = bpf_mixture_component;

// What mixtureFromHits returns: the components, the row each came from and the rows each one suppressed
struct PoseMixture
{
  std::vector<MixtureComponent> components;
  std::vector<int> source_row;
  std::vector<int> merged;

  // The rotation and sigma (with take_mean also the mean) of every component from the row of `moments` (poseMoments
  // of the rows the mixture was made from) it came from: eigenvectors and clamped eigenvalues of the row's covariance;
  // a component whose row is invalid keeps what it had.  Host code, no engine: bpf_pose_mixture_apply_moments.
  void mixtureApplyMoments(const std::vector<bpf_pose_moments>& moments, const std::array<double, 3>& sigma_floor,
                           const std::array<double, 3>& sigma_cap, bool take_mean = false)
  {
    const int rc = bpf_pose_mixture_apply_moments(components.data(), (int)components.size(), source_row.data(),
                                                  moments.data(), (int)moments.size(), sigma_floor.data(),
                                                  sigma_cap.data(), take_mean ? 1 : 0);
    if (rc != BPF_OK)
      throw std::runtime_error(std::string("bpf_pose_mixture_apply_moments: ") + bpf_error_string(rc));
  }
};

// Mixture components from pose-search hits or refined rows (bpf_pose_hit, bpf_pose_refined: anything with .pose and
// .score): the best rows by score, rows within the merge distances of a better one suppressed, total_count samples
// shared out by score.  Host code, no engine: bpf_pose_mixture_from_hits.
template <class Row>
inline PoseMixture mixtureFromHits(const std::vector<Row>& rows, int total_count, double xy_merge, double theta_merge,
                                   int max_components, const std::array<double, 3>& sigma)
{
  std::vector<double> xyt, scores;
  for (const Row& r : rows)
  {
    xyt.insert(xyt.end(), r.pose, r.pose + 3);
    scores.push_back(r.score);
  }
  const size_t cap = (size_t)(max_components > 0 ? max_components : 1);
  PoseMixture m;
  m.components.resize(cap);
  m.source_row.resize(cap);
  m.merged.resize(cap);
  int n = 0;
  const int rc = bpf_pose_mixture_from_hits(xyt.data(), scores.data(), (int)rows.size(), total_count, xy_merge,
                                            theta_merge, max_components, sigma.data(), m.components.data(),
                                            m.source_row.data(), m.merged.data(), &n);
  if (rc != BPF_OK)
    throw std::runtime_error(std::string("bpf_pose_mixture_from_hits: ") + bpf_error_string(rc));
  m.components.resize((size_t)n);
  m.source_row.resize((size_t)n);
  m.merged.resize((size_t)n);
  return m;
}

struct PFSampleSet
{
  int sample_count = 0;
  std::vector<PFSample> samples;
  int converged = 0;
  int leaf_count = 0;
};

class OccupancyMap
{
public:
  OccupancyMap(std::shared_ptr<Engine> e, double resolution) : e_(std::move(e)), resolution_(resolution) {}
  void setOrigin(float x, float y) { ox_ = x; oy_ = y; dirty_ = true; }
  std::vector<int> getSize() const { return { size_x_, size_y_ }; }
  void setSize(const std::vector<int>& size_vec)
  {
    size_x_ = size_vec[0];
    size_y_ = size_vec[1];
    cells_.assign((size_t)size_x_ * size_y_, CELL_UNKNOWN);
    dirty_ = true;
  }
  unsigned computeCellIndex(int i, int j) const { return i + j * unsigned(size_x_); }
  void setCellState(int index, MapCellState s) { cells_[index] = s; dirty_ = true; }
  MapCellState getCellState(int i, int j) const { return (MapCellState)cells_[computeCellIndex(i, j)]; }
  bool isValid(const std::vector<int>& c) const { return c[0] >= 0 && c[0] < size_x_ && c[1] >= 0 && c[1] < size_y_; }
  // adopt a host-built distances_lut_ (e.g. the reference's brushfire result)
  void setDistancesLUT(const std::vector<float>& lut, double max_distance_to_object)
  {
    lut_ = lut;
    max_dist_ = max_distance_to_object;
    dirty_ = true;
  }
  // OccupancyMap::updateDistancesLUT (occupancy_map.cpp:138-252): the reference's own priority-queue brushfire, the
  // reference's values bit for bit (host, once per map as in the reference, ~0.45 s per 2000^2 map)
  void updateDistancesLUT(double max_distance_to_object)
  {
    upload();
    e_->check(bpf_map2d_build_distances_lut_reference(e_->get(), max_distance_to_object));
    max_dist_ = max_distance_to_object;
    lut_.clear();
  }
  void updateDistancesLUTReference(double max_distance_to_object) { updateDistancesLUT(max_distance_to_object); }
  // NOT a reference method: the exact capped Euclidean distance transform, built on the device in milliseconds.  Its
  // values are <= the brushfire's and differ from them in < 1 % of the cells, so weights differ from the reference's
  // for particles whose beams end there -- an explicit choice of the caller (badger_pf.h, BPF_OPT_LUT_EXACT_EDT)
  void updateDistancesLUTExact(double max_distance_to_object)
  {
    upload();
    e_->check(bpf_map2d_build_distances_lut(e_->get(), max_distance_to_object));
    max_dist_ = max_distance_to_object;
    lut_.clear();
  }
  double getMaxDistanceToObject() const { return max_dist_; }
  // distances_lut_ as the engine holds it (index i + j * size_x, occupancy_map.cpp:107-110)
  std::vector<float> getDistancesLUT()
  {
    upload();
    std::vector<float> out((size_t)size_x_ * size_y_);
    e_->check(bpf_map2d_get_distances_lut(e_->get(), out.data(), out.size()));
    return out;
  }
  // OccupancyMap::calcRange (occupancy_map.cpp:257-364); cos / sin from libm here, as the reference forms them
  double calcRange(double ox, double oy, double oa, double max_range)
  {
    upload();
    const double ca = std::cos(oa), sa = std::sin(oa);
    double out = 0.0;
    e_->check(bpf_map2d_calc_range(e_->get(), &ox, &oy, &ca, &sa, &max_range, 1, &out));
    return out;
  }
  void upload()
  {
    if (!dirty_)
      return;
    e_->check(bpf_map2d_set(e_->get(), cells_.data(), lut_.empty() ? nullptr : lut_.data(), size_x_, size_y_, ox_, oy_,
                            resolution_, max_dist_));
    dirty_ = false;
  }

private:
  std::shared_ptr<Engine> e_;
  double resolution_;
  int size_x_ = 0, size_y_ = 0;
  float ox_ = 0, oy_ = 0;
  double max_dist_ = 0;
  std::vector<int32_t> cells_;
  std::vector<float> lut_;
  bool dirty_ = true;
};

struct PlanarData
{
  int range_count_ = 0;
  double range_max_ = 0;
  std::vector<double> ranges_, angles_;
};

class ParticleFilter
{
public:
  ParticleFilter(std::shared_ptr<Engine> e, int min_samples, int max_samples, double alpha_slow, double alpha_fast,
                 double global_localization_convergence_threshold)
      : e_(std::move(e)), max_samples_(max_samples)
  {
    e_->check(bpf_pf_create(e_->get(), min_samples, max_samples, alpha_slow, alpha_fast,
                            global_localization_convergence_threshold));
  }
  void setResampleModel(PFResampleModelType m) { e_->check(bpf_pf_set_resample_model(e_->get(), m)); }
  // random_pose_fn of the reference's constructor: true = Node::randomFreeSpacePose on the device (badger_pf.h)
  // three_d: over Node3D::updateFreeSpaceIndices (the 3-D map's column rectangle) instead of Node2D's list
  void setRandomFreeSpacePoseGenerator(bool on, bool three_d = false)
  {
    e_->check(bpf_pf_set_random_pose_generator(
        e_->get(), !on ? BPF_RANDOM_POSE_NONE : three_d ? BPF_RANDOM_POSE_FREE_SPACE_3D : BPF_RANDOM_POSE_FREE_SPACE_2D));
  }
  // Node::uniformPoseGenerator's score check (uniform_pose_starting_weight_threshold, uniform_pose_deweight_multiplier)
  void setUniformPoseCheck(double starting_weight_threshold, double deweight_multiplier,
                           int scoring = BPF_POSE_CHECK_AS_REFERENCE)
  {
    e_->check(bpf_pf_set_uniform_pose_check(e_->get(), starting_weight_threshold, deweight_multiplier, scoring));
  }
  // what the KLD stop rule counts: BPF_KLD_COUNT_LEAVES (default, the reference's) or BPF_KLD_COUNT_BINS (distinct
  // histogram bins, parity unpinned by construction); see bpf_pf_set_kld_count
  void setKldCount(int mode) { e_->check(bpf_pf_set_kld_count(e_->get(), mode)); }
  int getKldCount() const
  {
    int mode = BPF_KLD_COUNT_LEAVES;
    e_->check(bpf_pf_get_kld_count(e_->get(), &mode));
    return mode;
  }
  void setPopulationSizeParameters(double pop_err, double pop_z)
  {
    e_->check(bpf_pf_set_population_size_parameters(e_->get(), pop_err, pop_z));
  }
  void setDecayRates(double a_slow, double a_fast) { e_->check(bpf_pf_set_decay_rates(e_->get(), a_slow, a_fast)); }
  void srand48(long seed) { e_->check(bpf_pf_srand48(e_->get(), seed)); }
  // initWithPoseFn: pose_fn() returns {x, y, theta}
  template <typename PoseFn>
  void initWithPoseFn(PoseFn pose_fn)
  {
    std::vector<PFSample> s(max_samples_);
    for (auto& p : s)
    {
      p.pose = pose_fn();
      p.weight = 1.0 / max_samples_;
    }
    initWithSamples(s);
  }
  void initWithSamples(const std::vector<PFSample>& s, int leaf_count = -1)
  {
    e_->check(bpf_pf_set_samples(e_->get(), reinterpret_cast<const double*>(s.data()), (int)s.size(), leaf_count));
  }
  // ParticleFilter::initWithGaussian given PDFGaussian's decomposition (cr_ row-major 3x3, cd_), and
  // ParticleFilter::initWithPoseFn with the generator of setRandomFreeSpacePoseGenerator (global localisation)
  void initWithGaussian(const std::array<double, 3>& mean, const std::array<double, 9>& rotation,
                        const std::array<double, 3>& sigma)
  {
    e_->check(bpf_pf_init_with_gaussian(e_->get(), mean.data(), rotation.data(), sigma.data()));
  }
  void initWithRandomPoses() { e_->check(bpf_pf_init_with_random_poses(e_->get())); }
  // K Gaussian components, component k taking count_k consecutive samples from the filter's one drand48 stream (the
  // counts sum to max_samples).  Not a reference call for K > 1; K = 1 is initWithGaussian.
  void initWithMixture(const std::vector<MixtureComponent>& components)
  {
    e_->check(bpf_pf_init_with_mixture(e_->get(), components.data(), (int)components.size()));
  }
  int maxSamples() const { return max_samples_; }
  void updateResample() { e_->check(bpf_pf_update_resample(e_->get())); }
  std::shared_ptr<PFSampleSet> getCurrentSet()
  {
    auto set = std::make_shared<PFSampleSet>();
    set->samples.resize(max_samples_);
    int n = 0;
    e_->check(bpf_pf_get_samples(e_->get(), reinterpret_cast<double*>(set->samples.data()), max_samples_, &n));
    set->samples.resize(n);
    bpf_pf_state st;
    e_->check(bpf_pf_get_state(e_->get(), &st));
    set->sample_count = n;
    set->converged = st.converged;
    set->leaf_count = st.leaf_count;
    return set;
  }
  bool isConverged()
  {
    bpf_pf_state st;
    e_->check(bpf_pf_get_state(e_->get(), &st));
    return st.converged != 0;
  }
  bpf_pf_state getState()
  {
    bpf_pf_state st;
    e_->check(bpf_pf_get_state(e_->get(), &st));
    return st;
  }
  // ParticleFilter::getClusterStats(cidx, &weight, &mean) (particle_filter.cpp:638-649)
  bool getClusterStats(int cidx, double* weight, std::array<double, 3>* mean)
  {
    bpf_cluster c;
    const int rc = bpf_pf_get_cluster(e_->get(), cidx, &c);
    if (rc == BPF_ERR_INVALID_ARGUMENT)
      return false;
    e_->check(rc);
    *weight = c.weight;
    *mean = { c.mean[0], c.mean[1], c.mean[2] };
    return true;
  }
  // Node2D::getMaxWeightPose (node_2d.cpp:588-617)
  void getMaxWeightPose(double* max_weight_out, std::array<double, 3>* max_pose)
  {
    double pose[3] = { 0, 0, 0 };
    e_->check(bpf_pf_get_max_weight_pose(e_->get(), max_weight_out, pose));
    *max_pose = { pose[0], pose[1], pose[2] };
  }
  // Node::publishParticleCloud's poses (node.cpp:335-357) formed on the device: *poses7 ends as count x
  // {x, y, 0, qx, qy, qz, qw} of samples first, first + stride, ...  A vector that keeps its storage between calls can
  // be registered once (bpf_host_buffer_register on poses7->data(), again only when it grows): the copy engine then
  // writes it directly.
  void getPoseArray(std::vector<double>* poses7, int first = 0, int stride = 1)
  {
    bpf_pf_state st;
    e_->check(bpf_pf_get_state(e_->get(), &st));
    const long long n = st.sample_count;
    const long long room = (stride >= 1 && first >= 0 && first < n) ? (n - first + stride - 1) / stride : 0;
    if (poses7->size() < (size_t)(7 * room + 7))
      poses7->resize((size_t)(7 * room + 7));  // (never an empty vector: data() must be an address)
    int count = 0;
    e_->check(bpf_pf_get_pose_array(e_->get(), first, stride, poses7->data(), (int)room, &count));
    poses7->resize((size_t)7 * (size_t)count);
  }
  Engine& engine() { return *e_; }

private:
  std::shared_ptr<Engine> e_;
  int max_samples_;
};

enum OdomModelType
{
  ODOM_MODEL_DIFF = BPF_ODOM_MODEL_DIFF,
  ODOM_MODEL_OMNI = BPF_ODOM_MODEL_OMNI,
  ODOM_MODEL_DIFF_CORRECTED = BPF_ODOM_MODEL_DIFF_CORRECTED,
  ODOM_MODEL_OMNI_CORRECTED = BPF_ODOM_MODEL_OMNI_CORRECTED,
  ODOM_MODEL_GAUSSIAN = BPF_ODOM_MODEL_GAUSSIAN
};

struct OdomData
{
  std::array<double, 3> pose{}, delta{}, absolute_motion{};
};

class Odom
{
public:
  explicit Odom(std::shared_ptr<Engine> e) : e_(std::move(e)) {}
  void setModel(OdomModelType type, double alpha1, double alpha2, double alpha3, double alpha4, double alpha5 = 0)
  {
    e_->check(bpf_odom_set_model(e_->get(), type, alpha1, alpha2, alpha3, alpha4, alpha5));
  }
  bool updateAction(std::shared_ptr<ParticleFilter>, std::shared_ptr<OdomData> data)
  {
    e_->check(bpf_pf_update_action(e_->get(), data->pose.data(), data->delta.data(), data->absolute_motion.data()));
    return true;
  }

private:
  std::shared_ptr<Engine> e_;
};

class PlanarScanner
{
public:
  explicit PlanarScanner(std::shared_ptr<Engine> e) : e_(std::move(e))
  {
    e_->check(bpf_planar_set_map_factors(e_->get(), 1.0, 1.0, 0.0));  // planar_scanner.cpp:42-44
  }
  void init(int max_beams, std::shared_ptr<OccupancyMap> map)
  {
    max_beams_ = max_beams;
    map_ = std::move(map);
    map_->upload();
    e_->check(bpf_planar_init(e_->get(), max_beams));
  }
  void setModelBeam(double z_hit, double z_short, double z_max, double z_rand, double sigma_hit, double lambda_short)
  {
    map_->upload();
    e_->check(bpf_planar_set_model_beam(e_->get(), z_hit, z_short, z_max, z_rand, sigma_hit, lambda_short));
  }
  void setModelLikelihoodField(double z_hit, double z_rand, double sigma_hit, double max_distance_to_object)
  {
    map_->upload();
    e_->check(bpf_planar_set_model_likelihood_field(e_->get(), z_hit, z_rand, sigma_hit, max_distance_to_object));
  }
  void setModelLikelihoodFieldProb(double z_hit, double z_rand, double sigma_hit, double max_distance_to_object,
                                   bool do_beamskip, double beam_skip_distance, double beam_skip_threshold,
                                   double beam_skip_error_threshold)
  {
    map_->upload();
    e_->check(bpf_planar_set_model_likelihood_field_prob(e_->get(), z_hit, z_rand, sigma_hit, max_distance_to_object,
                                                         do_beamskip, beam_skip_distance, beam_skip_threshold,
                                                         beam_skip_error_threshold));
  }
  void setModelLikelihoodFieldGompertz(double z_hit, double z_rand, double sigma_hit, double max_distance_to_object,
                                       double gompertz_a, double gompertz_b, double gompertz_c, double input_shift,
                                       double input_scale, double output_shift)
  {
    map_->upload();
    e_->check(bpf_planar_set_model_likelihood_field_gompertz(e_->get(), z_hit, z_rand, sigma_hit,
                                                             max_distance_to_object, gompertz_a, gompertz_b,
                                                             gompertz_c, input_shift, input_scale, output_shift));
  }
  void setMapFactors(double off_map_factor, double non_free_space_factor, double non_free_space_radius)
  {
    e_->check(bpf_planar_set_map_factors(e_->get(), off_map_factor, non_free_space_factor, non_free_space_radius));
  }
  void setPlanarScannerPose(const std::array<double, 3>& pose) { e_->check(bpf_planar_set_scanner_pose(e_->get(), pose.data())); }

  // PlanarScanner::updateSensor(pf, data): false and no effect when max_beams_ < 2
  bool updateSensor(std::shared_ptr<ParticleFilter> pf, std::shared_ptr<PlanarData> data)
  {
    if (max_beams_ < 2)
      return false;
    e_->check(bpf_pf_update_sensor_planar(e_->get(), data->ranges_.data(), data->angles_.data(), data->range_count_,
                                          data->range_max_));
    (void)pf;
    return true;
  }
  // PlanarScanner::applyModelToSampleSet(data, set) on a host-resident set
  double applyModelToSampleSet(std::shared_ptr<PlanarData> data, std::shared_ptr<PFSampleSet> set)
  {
    int status = BPF_OK;
    const double total = bpf_planar_apply_model_to_sample_set(
        e_->get(), reinterpret_cast<double*>(set->samples.data()), set->sample_count, set->converged,
        data->ranges_.data(), data->angles_.data(), data->range_count_, data->range_max_, &status);
    e_->check(status);
    return total;
  }

  // NOT a reference method (bpf_planar_search_poses): every free cell of the map (every cell_stride-th in i and j) at
  // `headings` headings scored against `data` on the device; the best k of candidates first .. first + count - 1
  // (count = -1: to the end), score descending, equal scores by candidate.  A global-localisation service turns the
  // hits into a sample set (ParticleFilter::initWithSamples).
  std::vector<bpf_pose_hit> searchPoses(std::shared_ptr<PlanarData> data, int headings, int cell_stride, int k,
                                        long long first = 0, long long count = -1)
  {
    if (map_)
      map_->upload();
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e_->check(bpf_planar_search_poses(e_->get(), data->ranges_.data(), data->angles_.data(), data->range_count_,
                                      data->range_max_, headings, cell_stride, first, count, k, hits.data(), &n));
    hits.resize((size_t)n);
    return hits;
  }
  // NOT a reference method (bpf_planar_search_poses_joint): searchPoses over several scans.  Scan s is scored at the
  // candidate's pose composed with offsets[s] = (dx, dy, dth) -- the robot's pose at scan s in the frame of the
  // candidate pose, an odometry delta --, the weight carried from scan to scan; the rows carry the BASE pose.
  std::vector<bpf_pose_hit> searchPosesJoint(const std::vector<std::shared_ptr<PlanarData>>& datas,
                                             const std::vector<std::array<double, 3>>& offsets, int headings,
                                             int cell_stride, int k, long long first = 0, long long count = -1)
  {
    if (datas.size() != offsets.size())
      throw std::invalid_argument("searchPosesJoint: one offset per scan is needed");
    if (map_)
      map_->upload();
    std::vector<const double*> ranges, angles;
    std::vector<int> counts;
    std::vector<double> maxes, off;
    for (size_t s = 0; s < datas.size(); ++s)
    {
      ranges.push_back(datas[s]->ranges_.data());
      angles.push_back(datas[s]->angles_.data());
      counts.push_back(datas[s]->range_count_);
      maxes.push_back(datas[s]->range_max_);
      off.insert(off.end(), offsets[s].begin(), offsets[s].end());
    }
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e_->check(bpf_planar_search_poses_joint(e_->get(), (int)datas.size(), ranges.data(), angles.data(), counts.data(),
                                            maxes.data(), off.data(), headings, cell_stride, first, count, k,
                                            hits.data(), &n));
    hits.resize((size_t)n);
    return hits;
  }
  // NOT a reference method (bpf_planar_search_poses_pruned): the rows of searchPoses over the candidates whose cells
  // lie in blocks first_block .. first_block + block_count - 1 (block_count = -1: to the end) of the list of
  // block x block cell blocks, bit for bit, from fewer exact evaluations.  Likelihood field and Gompertz only.
  std::vector<bpf_pose_hit> searchPosesPruned(std::shared_ptr<PlanarData> data, int headings, int cell_stride, int k,
                                              int block = 8, int first_block = 0, int block_count = -1,
                                              bpf_pose_search_stats* stats_out = nullptr)
  {
    if (map_)
      map_->upload();
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e_->check(bpf_planar_search_poses_pruned(e_->get(), data->ranges_.data(), data->angles_.data(),
                                             data->range_count_, data->range_max_, headings, cell_stride, block,
                                             first_block, block_count, k, hits.data(), &n, stats_out));
    hits.resize((size_t)n);
    return hits;
  }
  // blocks in that list: what a caller of searchPosesPruned splits into ranges
  int searchBlocks(int cell_stride = 1, int block = 8)
  {
    if (map_)
      map_->upload();
    int n = 0;
    e_->check(bpf_planar_search_blocks(e_->get(), cell_stride, block, &n));
    return n;
  }
  // NOT a reference method (bpf_planar_refine_poses): coarse-to-fine lattice descent around every pose of `poses_xyt`
  // (x, y, theta triples) against `data` on the device; row r refines pose r.  trace_out, when given, receives the
  // lattice point chosen per (pose, level), poses.size() / 3 * levels ints.
  std::vector<bpf_pose_refined> refinePoses(std::shared_ptr<PlanarData> data, const std::vector<double>& poses_xyt,
                                            int xy_radius, double xy_step, int theta_radius, double theta_step,
                                            int levels, std::vector<int>* trace_out = nullptr)
  {
    if (map_)
      map_->upload();
    const int n = (int)(poses_xyt.size() / 3);
    std::vector<bpf_pose_refined> rows((size_t)(n > 0 ? n : 1));
    if (trace_out)
      trace_out->assign((size_t)(n > 0 ? n : 1) * (size_t)(levels > 0 ? levels : 1), 0);
    e_->check(bpf_planar_refine_poses(e_->get(), data->ranges_.data(), data->angles_.data(), data->range_count_,
                                      data->range_max_, poses_xyt.data(), n, xy_radius, xy_step, theta_radius,
                                      theta_step, levels, rows.data(), trace_out ? trace_out->data() : nullptr));
    rows.resize((size_t)n);
    return rows;
  }
  // the same around the poses of a search's hits
  std::vector<bpf_pose_refined> refinePoses(std::shared_ptr<PlanarData> data, const std::vector<bpf_pose_hit>& hits,
                                            int xy_radius, double xy_step, int theta_radius, double theta_step,
                                            int levels, std::vector<int>* trace_out = nullptr)
  {
    return refinePoses(data, posesOfHits(hits), xy_radius, xy_step, theta_radius, theta_step, levels, trace_out);
  }
  // NOT a reference method (bpf_planar_pose_moments): the score-weighted first and second moments of one refinement
  // lattice (steps as given) around every pose of `poses_xyt` (x, y, theta triples) against `data` on the device; row
  // r describes pose r.  scores_out, when given, receives the lattice scores, poses.size() / 3 * M doubles.
  std::vector<bpf_pose_moments> poseMoments(std::shared_ptr<PlanarData> data, const std::vector<double>& poses_xyt,
                                            int xy_radius, double xy_step, int theta_radius, double theta_step,
                                            double baseline, std::vector<double>* scores_out = nullptr)
  {
    if (map_)
      map_->upload();
    const int n = (int)(poses_xyt.size() / 3);
    std::vector<bpf_pose_moments> rows((size_t)(n > 0 ? n : 1));
    if (scores_out)
      scores_out->assign((size_t)(n > 0 ? n : 1) * latticePoints(xy_radius, theta_radius), 0.0);
    e_->check(bpf_planar_pose_moments(e_->get(), data->ranges_.data(), data->angles_.data(), data->range_count_,
                                      data->range_max_, poses_xyt.data(), n, xy_radius, xy_step, theta_radius,
                                      theta_step, baseline, rows.data(), scores_out ? scores_out->data() : nullptr));
    rows.resize((size_t)n);
    return rows;
  }
  // the same around the poses of a search's hits or of refined rows
  std::vector<bpf_pose_moments> poseMoments(std::shared_ptr<PlanarData> data, const std::vector<bpf_pose_hit>& hits,
                                            int xy_radius, double xy_step, int theta_radius, double theta_step,
                                            double baseline, std::vector<double>* scores_out = nullptr)
  {
    return poseMoments(data, posesOfHits(hits), xy_radius, xy_step, theta_radius, theta_step, baseline, scores_out);
  }
  std::vector<bpf_pose_moments> poseMoments(std::shared_ptr<PlanarData> data,
                                            const std::vector<bpf_pose_refined>& refined, int xy_radius,
                                            double xy_step, int theta_radius, double theta_step, double baseline,
                                            std::vector<double>* scores_out = nullptr)
  {
    return poseMoments(data, posesOfRefined(refined), xy_radius, xy_step, theta_radius, theta_step, baseline,
                       scores_out);
  }
  // M of a lattice for sizing a score buffer (1 where the library would refuse the radii)
  static size_t latticePoints(int xy_radius, int theta_radius)
  {
    int m = 1;
    return bpf_pose_refine_lattice(xy_radius, theta_radius, &m, nullptr) == BPF_OK ? (size_t)m : 1;
  }
  static std::vector<double> posesOfRefined(const std::vector<bpf_pose_refined>& rows)
  {
    std::vector<double> xyt;
    xyt.reserve(rows.size() * 3);
    for (const auto& r : rows)
      xyt.insert(xyt.end(), r.pose, r.pose + 3);
    return xyt;
  }
  // x, y, theta of every hit, packed
  static std::vector<double> posesOfHits(const std::vector<bpf_pose_hit>& hits)
  {
    std::vector<double> xyt;
    xyt.reserve(hits.size() * 3);
    for (const auto& h : hits)
      xyt.insert(xyt.end(), h.pose, h.pose + 3);
    return xyt;
  }
  // candidates (free cells kept by cell_stride x headings) of searchPoses: what a caller splits into ranges
  long long searchSpace(int headings, int cell_stride = 1, int* free_cells_out = nullptr)
  {
    if (map_)
      map_->upload();
    long long total = 0;
    e_->check(bpf_planar_search_space(e_->get(), headings, cell_stride, &total, free_cells_out));
    return total;
  }
  // the best k of the hit lists of disjoint ranges, in searchPoses' order (host code, no engine)
  static std::vector<bpf_pose_hit> mergePoseHits(const std::vector<std::vector<bpf_pose_hit>>& lists, int k)
  {
    std::vector<bpf_pose_hit> flat;
    std::vector<int> lengths;
    for (const auto& l : lists)
    {
      flat.insert(flat.end(), l.begin(), l.end());
      lengths.push_back((int)l.size());
    }
    std::vector<bpf_pose_hit> out((size_t)(k > 0 ? k : 1));
    int n = 0;
    const int rc = bpf_pose_search_merge(flat.data(), lengths.data(), (int)lists.size(), k, out.data(), &n);
    if (rc != BPF_OK)
      throw std::runtime_error(std::string("bpf_pose_search_merge: ") + bpf_error_string(rc));
    out.resize((size_t)n);
    return out;
  }

private:
  std::shared_ptr<Engine> e_;
  std::shared_ptr<OccupancyMap> map_;
  int max_beams_ = 0;
};

// LUT state of the reference's OctoMap (include/amcl/map/octomap.h:96-110): pose_indices_, distance_ratios_ and the
// cropped cell bounds.  Building it from an octree is the caller's job: either the finished LUT is adopted, or the
// engine builds it from the occupied voxels' indices.
class OctoMap
{
public:
  OctoMap(std::shared_ptr<Engine> e, double resolution) : e_(std::move(e)), resolution_(resolution) {}
  // adopt a host-built LUT: pose_indices (one per column of the bounds, j-major) and distance_ratios
  void setDistancesLUT(const std::vector<uint32_t>& pose_indices, const std::vector<uint8_t>& distance_ratios,
                       const std::array<int, 3>& min_cells, const std::array<int, 3>& max_cells,
                       double max_distance_to_object)
  {
    e_->check(bpf_map3d_set(e_->get(), pose_indices.data(), pose_indices.size(), distance_ratios.data(),
                            distance_ratios.size(), min_cells.data(), max_cells.data(), resolution_,
                            max_distance_to_object));
    adopt(min_cells, max_cells, max_distance_to_object);
  }
  // OctoMap::updateDistancesLUT (octomap.cpp:175-333) from the occupied voxels' indices, i j k packed, in octree leaf
  // order
  void updateDistancesLUT(const std::vector<int>& occupied_ijk, const std::array<int, 3>& min_cells,
                          const std::array<int, 3>& max_cells, double max_distance_to_object)
  {
    e_->check(bpf_map3d_build_distances_lut(e_->get(), occupied_ijk.data(), occupied_ijk.size() / 3, min_cells.data(),
                                            max_cells.data(), resolution_, max_distance_to_object));
    adopt(min_cells, max_cells, max_distance_to_object);
  }
  // pose_indices_ and distance_ratios_ as the engine holds them
  void getDistancesLUT(std::vector<uint32_t>* pose_indices, std::vector<uint8_t>* distance_ratios)
  {
    size_t n_pose = 0, n_ratios = 0;
    e_->check(bpf_map3d_get_distances_lut(e_->get(), nullptr, 0, &n_pose, nullptr, 0, &n_ratios));
    pose_indices->resize(n_pose);
    distance_ratios->resize(n_ratios);
    e_->check(bpf_map3d_get_distances_lut(e_->get(), pose_indices->data(), n_pose, nullptr, distance_ratios->data(),
                                          n_ratios, nullptr));
  }
  double getMaxDistanceToObject() const { return max_dist_; }
  double getResolution() const { return resolution_; }
  std::array<int, 3> getMinCells() const { return min_cells_; }
  std::array<int, 3> getMaxCells() const { return max_cells_; }

private:
  void adopt(const std::array<int, 3>& min_cells, const std::array<int, 3>& max_cells, double max_dist)
  {
    min_cells_ = min_cells;
    max_cells_ = max_cells;
    max_dist_ = max_dist;
  }
  std::shared_ptr<Engine> e_;
  double resolution_;
  double max_dist_ = 0;
  std::array<int, 3> min_cells_{}, max_cells_{};
};

// include/amcl/sensors/point_cloud_scanner.h:45-51; points_: packed float xyz in the scanner frame
struct PointCloudData
{
  std::vector<float> points_;
  int pointCount() const { return (int)(points_.size() / 3); }
};

// include/amcl/sensors/point_cloud_scanner.h:53-120
class PointCloudScanner
{
public:
  explicit PointCloudScanner(std::shared_ptr<Engine> e) : e_(std::move(e)) {}
  void init(int max_beams, std::shared_ptr<OctoMap> map)
  {
    max_beams_ = max_beams;
    map_ = std::move(map);
    e_->check(bpf_cloud_init(e_->get(), max_beams));
  }
  void setPointCloudModel(double z_hit, double z_rand, double sigma_hit)
  {
    e_->check(bpf_cloud_set_model(e_->get(), z_hit, z_rand, sigma_hit));
  }
  void setPointCloudModelGompertz(double z_hit, double z_rand, double sigma_hit, double gompertz_a, double gompertz_b,
                                  double gompertz_c, double input_shift, double input_scale, double output_shift)
  {
    e_->check(bpf_cloud_set_model_gompertz(e_->get(), z_hit, z_rand, sigma_hit, gompertz_a, gompertz_b, gompertz_c,
                                           input_shift, input_scale, output_shift));
  }
  void setMapFactors(double off_map_factor, double non_free_space_factor, double non_free_space_radius)
  {
    e_->check(bpf_cloud_set_map_factors(e_->get(), off_map_factor, non_free_space_factor, non_free_space_radius));
  }
  // translation and rotation (quaternion x y z w) of the scanner in the robot's footprint frame
  void setPointCloudScannerToFootprintTF(const std::array<double, 3>& xyz, const std::array<double, 4>& quat_xyzw)
  {
    e_->check(bpf_cloud_set_scanner_to_footprint_tf(e_->get(), xyz.data(), quat_xyzw.data()));
  }

  // PointCloudScanner::updateSensor(pf, data): false and no effect when max_beams_ < 2
  bool updateSensor(std::shared_ptr<ParticleFilter> pf, std::shared_ptr<PointCloudData> data)
  {
    if (max_beams_ < 2)
      return false;
    e_->check(bpf_pf_update_sensor_cloud(e_->get(), data->points_.data(), data->pointCount()));
    (void)pf;
    return true;
  }
  // PointCloudScanner::applyModelToSampleSet(data, set) on a host-resident set
  double applyModelToSampleSet(std::shared_ptr<PointCloudData> data, std::shared_ptr<PFSampleSet> set)
  {
    int status = BPF_OK;
    const double total = bpf_cloud_apply_model_to_sample_set(e_->get(), reinterpret_cast<double*>(set->samples.data()),
                                                             set->sample_count, data->points_.data(),
                                                             data->pointCount(), &status);
    e_->check(status);
    return total;
  }

  // NOT a reference method (bpf_cloud_search_poses): every column of the 3-D map's rectangle (every cell_stride-th in
  // i and j) at `headings` headings scored against `data` on the device; the best k of candidates first ..
  // first + count - 1 (count = -1: to the end), score descending, equal scores by candidate.  A Node3D's global
  // localisation turns the hits into a sample set (ParticleFilter::initWithSamples).
  std::vector<bpf_pose_hit> searchPoses(std::shared_ptr<PointCloudData> data, int headings, int cell_stride, int k,
                                        long long first = 0, long long count = -1)
  {
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e_->check(bpf_cloud_search_poses(e_->get(), data->points_.data(), data->pointCount(), headings, cell_stride, first,
                                     count, k, hits.data(), &n));
    hits.resize((size_t)n);
    return hits;
  }
  // NOT a reference method (bpf_cloud_search_poses_joint): searchPoses over several clouds.  Cloud s is scored at the
  // candidate's pose composed with offsets[s] = (dx, dy, dth) -- the robot's pose at cloud s in the frame of the
  // candidate pose, an odometry delta --, the weight carried from cloud to cloud; the rows carry the BASE pose.
  std::vector<bpf_pose_hit> searchPosesJoint(const std::vector<std::shared_ptr<PointCloudData>>& datas,
                                             const std::vector<std::array<double, 3>>& offsets, int headings,
                                             int cell_stride, int k, long long first = 0, long long count = -1)
  {
    if (datas.size() != offsets.size())
      throw std::invalid_argument("searchPosesJoint: one offset per cloud is needed");
    std::vector<const float*> points;
    std::vector<int> counts;
    std::vector<double> off;
    for (size_t s = 0; s < datas.size(); ++s)
    {
      points.push_back(datas[s]->points_.data());
      counts.push_back(datas[s]->pointCount());
      off.insert(off.end(), offsets[s].begin(), offsets[s].end());
    }
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e_->check(bpf_cloud_search_poses_joint(e_->get(), (int)datas.size(), points.data(), counts.data(), off.data(),
                                           headings, cell_stride, first, count, k, hits.data(), &n));
    hits.resize((size_t)n);
    return hits;
  }
  // NOT a reference method (bpf_cloud_search_poses_pruned): the rows of searchPoses over the candidates whose columns
  // lie in blocks first_block .. first_block + block_count - 1 (block_count = -1: to the end) of the list of
  // block x block column blocks, bit for bit, from fewer exact evaluations.  A mounting without roll or pitch and a
  // map with the dense volume only.
  std::vector<bpf_pose_hit> searchPosesPruned(std::shared_ptr<PointCloudData> data, int headings, int cell_stride,
                                              int k, int block = 16, int first_block = 0, int block_count = -1,
                                              bpf_pose_search_stats* stats_out = nullptr)
  {
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e_->check(bpf_cloud_search_poses_pruned(e_->get(), data->points_.data(), data->pointCount(), headings, cell_stride,
                                            block, first_block, block_count, k, hits.data(), &n, stats_out));
    hits.resize((size_t)n);
    return hits;
  }
  // blocks in that list: what a caller of searchPosesPruned splits into ranges
  int searchBlocks(int cell_stride = 1, int block = 16)
  {
    int n = 0;
    e_->check(bpf_cloud_search_blocks(e_->get(), cell_stride, block, &n));
    return n;
  }
  // the bounds searchPosesPruned prunes with, of block candidates first_q .. first_q + count - 1 (count = -1: to the
  // end of the block list x headings).  For diagnosis and tests.
  std::vector<double> searchBounds(std::shared_ptr<PointCloudData> data, int headings, int cell_stride, int block = 16,
                                   long long first_q = 0, long long count = -1)
  {
    if (count < 0)
      count = (long long)searchBlocks(cell_stride, block) * headings - first_q;
    std::vector<double> bounds((size_t)(count > 0 ? count : 1));
    e_->check(bpf_cloud_search_bounds(e_->get(), data->points_.data(), data->pointCount(), headings, cell_stride, block,
                                      first_q, count, bounds.data()));
    bounds.resize((size_t)(count > 0 ? count : 0));
    return bounds;
  }
  // the pooled volume searchPosesPruned bounds with, in the engine's dense layout: planes of ntx x nty tiles of 64
  // bytes, the zero plane last.  For diagnosis and tests.
  std::vector<unsigned char> searchPooledLut(int block = 16, int* ntx_out = nullptr, int* nty_out = nullptr,
                                             int* planes_out = nullptr)
  {
    long long n = 0;
    e_->check(bpf_cloud_search_pooled_lut(e_->get(), block, nullptr, 0, &n, ntx_out, nty_out, planes_out));
    std::vector<unsigned char> bytes((size_t)n);
    e_->check(bpf_cloud_search_pooled_lut(e_->get(), block, bytes.data(), n, &n, ntx_out, nty_out, planes_out));
    return bytes;
  }
  // NOT a reference method (bpf_cloud_refine_poses): coarse-to-fine lattice descent around every pose of `poses_xyt`
  // (x, y, theta triples) against the cloud `data` on the device; row r refines pose r.  trace_out, when given,
  // receives the lattice point chosen per (pose, level), poses.size() / 3 * levels ints.
  std::vector<bpf_pose_refined> refinePoses(std::shared_ptr<PointCloudData> data, const std::vector<double>& poses_xyt,
                                            int xy_radius, double xy_step, int theta_radius, double theta_step,
                                            int levels, std::vector<int>* trace_out = nullptr)
  {
    const int n = (int)(poses_xyt.size() / 3);
    std::vector<bpf_pose_refined> rows((size_t)(n > 0 ? n : 1));
    if (trace_out)
      trace_out->assign((size_t)(n > 0 ? n : 1) * (size_t)(levels > 0 ? levels : 1), 0);
    e_->check(bpf_cloud_refine_poses(e_->get(), data->points_.data(), data->pointCount(), poses_xyt.data(), n,
                                     xy_radius, xy_step, theta_radius, theta_step, levels, rows.data(),
                                     trace_out ? trace_out->data() : nullptr));
    rows.resize((size_t)n);
    return rows;
  }
  // the same around the poses of a search's hits
  std::vector<bpf_pose_refined> refinePoses(std::shared_ptr<PointCloudData> data,
                                            const std::vector<bpf_pose_hit>& hits, int xy_radius, double xy_step,
                                            int theta_radius, double theta_step, int levels,
                                            std::vector<int>* trace_out = nullptr)
  {
    return refinePoses(data, PlanarScanner::posesOfHits(hits), xy_radius, xy_step, theta_radius, theta_step, levels,
                       trace_out);
  }
  // NOT a reference method (bpf_cloud_pose_moments): the score-weighted first and second moments of one refinement
  // lattice (steps as given) around every pose of `poses_xyt` against the cloud `data` on the device; row r describes
  // pose r.  scores_out, when given, receives the lattice scores, poses.size() / 3 * M doubles.
  std::vector<bpf_pose_moments> poseMoments(std::shared_ptr<PointCloudData> data, const std::vector<double>& poses_xyt,
                                            int xy_radius, double xy_step, int theta_radius, double theta_step,
                                            double baseline, std::vector<double>* scores_out = nullptr)
  {
    const int n = (int)(poses_xyt.size() / 3);
    std::vector<bpf_pose_moments> rows((size_t)(n > 0 ? n : 1));
    if (scores_out)
      scores_out->assign((size_t)(n > 0 ? n : 1) * PlanarScanner::latticePoints(xy_radius, theta_radius), 0.0);
    e_->check(bpf_cloud_pose_moments(e_->get(), data->points_.data(), data->pointCount(), poses_xyt.data(), n,
                                     xy_radius, xy_step, theta_radius, theta_step, baseline, rows.data(),
                                     scores_out ? scores_out->data() : nullptr));
    rows.resize((size_t)n);
    return rows;
  }
  // the same around the poses of a search's hits or of refined rows
  std::vector<bpf_pose_moments> poseMoments(std::shared_ptr<PointCloudData> data,
                                            const std::vector<bpf_pose_hit>& hits, int xy_radius, double xy_step,
                                            int theta_radius, double theta_step, double baseline,
                                            std::vector<double>* scores_out = nullptr)
  {
    return poseMoments(data, PlanarScanner::posesOfHits(hits), xy_radius, xy_step, theta_radius, theta_step, baseline,
                       scores_out);
  }
  std::vector<bpf_pose_moments> poseMoments(std::shared_ptr<PointCloudData> data,
                                            const std::vector<bpf_pose_refined>& refined, int xy_radius,
                                            double xy_step, int theta_radius, double theta_step, double baseline,
                                            std::vector<double>* scores_out = nullptr)
  {
    return poseMoments(data, PlanarScanner::posesOfRefined(refined), xy_radius, xy_step, theta_radius, theta_step,
                       baseline, scores_out);
  }
  // candidates (columns kept by cell_stride x headings) of searchPoses: what a caller splits into ranges
  long long searchSpace(int headings, int cell_stride = 1, int* columns_out = nullptr)
  {
    long long total = 0;
    e_->check(bpf_cloud_search_space(e_->get(), headings, cell_stride, &total, columns_out));
    return total;
  }
  // the best k of the hit lists of disjoint ranges, in searchPoses' order (host code, no engine)
  static std::vector<bpf_pose_hit> mergePoseHits(const std::vector<std::vector<bpf_pose_hit>>& lists, int k)
  {
    return PlanarScanner::mergePoseHits(lists, k);
  }

private:
  std::shared_ptr<Engine> e_;
  std::shared_ptr<OctoMap> map_;
  int max_beams_ = 0;
};

// One filter sharded over the GPUs of a node, this process being one rank of it (badger_pf.h, "sharded operation"):
// the engine holds this rank's contiguous slice and the GLOBAL min / max sample counts; every member below except the
// constructor is collective -- every rank calls it, in the same order.  The exchanges are the engine's own (mailbox
// peer stores, RCCL after the bootstrap's fallback); the class owns the figures the C calls pass back and forth.
class ShardedParticleFilter
{
public:
  // pf: this rank's filter; a slice loaded by hand comes with global_count (samples of the whole set), leaf_count (of
  // the whole set's histogram tree: only the systematic resampler reads it before the first resample) and global_first
  // (the global index of the slice's first sample: the motion update needs it).  A set started with initWithGaussian /
  // initWithRandomPoses needs none of the three.
  ShardedParticleFilter(std::shared_ptr<ParticleFilter> pf, int global_count, int leaf_count = 1, int first_window = 4096,
                        long long global_first = 0)
      : pf_(std::move(pf)), global_count_(global_count), leaf_count_(leaf_count), window_hint_(first_window),
        first_window_(first_window), global_first_(global_first)
  {
  }
  // host_port: "host:port" rank 0 listens on; max_window >= the filter's max_samples; flags: BPF_BOOTSTRAP_*;
  // returns BPF_SHARD_EXCHANGE_MAILBOX or BPF_SHARD_EXCHANGE_RCCL
  int bootstrap(int rank, int world, const std::string& host_port, long long max_window, int flags = 0)
  {
    int mode = 0;
    e().check(bpf_shard_bootstrap(e().get(), rank, world, host_port.c_str(), max_window, flags, &mode));
    rank_ = rank;
    world_ = world;
    return mode;
  }
  // ParticleFilter::initWithGaussian / initWithPoseFn over the shards (after bootstrap): this rank ends with its even
  // share of the max_samples samples one engine would hold, every rank with the same rng state and with the leaf /
  // bin counts of the whole set's histogram tree
  void initWithGaussian(const std::array<double, 3>& mean, const std::array<double, 9>& rotation,
                        const std::array<double, 3>& sigma)
  {
    e().check(bpf_shard_init_with_gaussian_all(e().get(), mean.data(), rotation.data(), sigma.data()));
    afterInit();
  }
  void initWithRandomPoses()
  {
    e().check(bpf_shard_init_with_random_poses_all(e().get()));
    afterInit();
  }
  void initWithMixture(const std::vector<MixtureComponent>& components)
  {
    e().check(bpf_shard_init_with_mixture_all(e().get(), components.data(), (int)components.size()));
    afterInit();
  }
  // Odom::updateAction on this rank's slice: no exchange, every rank ends on the same rng state
  bool updateAction(std::shared_ptr<OdomData> data)
  {
    e().check(bpf_shard_update_action(e().get(), data->pose.data(), data->delta.data(), data->absolute_motion.data(),
                                      global_first_, global_count_));
    return true;
  }
  // PlanarScanner::updateSensor over the shards (beam skipping of the prob model included)
  bool updateSensor(std::shared_ptr<PlanarData> data)
  {
    e().check(bpf_shard_update_sensor_planar(e().get(), data->ranges_.data(), data->angles_.data(), data->range_count_,
                                             data->range_max_, global_count_));
    return true;
  }
  // PointCloudScanner::updateSensor over the shards; xyz: n packed float triples in the scanner frame
  bool updateSensorCloud(const float* xyz, int n)
  {
    e().check(bpf_shard_update_sensor_cloud(e().get(), xyz, n, global_count_));
    return true;
  }
  // NOT reference methods (badger_pf.h, "pose search over a sharded filter"): PlanarScanner::searchPoses /
  // searchPosesPruned and PointCloudScanner's over the ranks.  The range given is split over the ranks, the ranks'
  // lists are merged on the device, and every rank returns the single engine's rows for the range, byte for byte.
  // The pruned forms share their tau behind the seed; stats_out counts this rank's share.
  std::vector<bpf_pose_hit> searchPoses(std::shared_ptr<PlanarData> data, int headings, int cell_stride, int k,
                                        long long first = 0, long long count = -1)
  {
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e().check(bpf_shard_search_poses(e().get(), data->ranges_.data(), data->angles_.data(), data->range_count_,
                                     data->range_max_, headings, cell_stride, first, count, k, hits.data(), &n));
    hits.resize((size_t)n);
    return hits;
  }
  std::vector<bpf_pose_hit> searchPosesPruned(std::shared_ptr<PlanarData> data, int headings, int cell_stride, int k,
                                              int block = 8, int first_block = 0, int block_count = -1,
                                              bpf_pose_search_stats* stats_out = nullptr)
  {
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e().check(bpf_shard_search_poses_pruned(e().get(), data->ranges_.data(), data->angles_.data(), data->range_count_,
                                            data->range_max_, headings, cell_stride, block, first_block, block_count,
                                            k, hits.data(), &n, stats_out));
    hits.resize((size_t)n);
    return hits;
  }
  std::vector<bpf_pose_hit> searchPosesCloud(const float* xyz, int n_points, int headings, int cell_stride, int k,
                                             long long first = 0, long long count = -1)
  {
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e().check(bpf_shard_cloud_search_poses(e().get(), xyz, n_points, headings, cell_stride, first, count, k,
                                           hits.data(), &n));
    hits.resize((size_t)n);
    return hits;
  }
  std::vector<bpf_pose_hit> searchPosesCloudPruned(const float* xyz, int n_points, int headings, int cell_stride,
                                                   int k, int block = 8, int first_block = 0, int block_count = -1,
                                                   bpf_pose_search_stats* stats_out = nullptr)
  {
    std::vector<bpf_pose_hit> hits((size_t)(k > 0 ? k : 1));
    int n = 0;
    e().check(bpf_shard_cloud_search_poses_pruned(e().get(), xyz, n_points, headings, cell_stride, block, first_block,
                                                  block_count, k, hits.data(), &n, stats_out));
    hits.resize((size_t)n);
    return hits;
  }
  // What localize() takes besides the search's arguments: the lattices of refinePoses and poseMoments, the clamps of
  // mixtureApplyMoments and the arguments of mixtureFromHits
  struct LocalizeSettings
  {
    int refine_xy_radius = 2, refine_theta_radius = 2, refine_levels = 2;
    double refine_xy_step = 0.025, refine_theta_step = 0.02;
    int moments_xy_radius = 2, moments_theta_radius = 2;
    double moments_xy_step = 0.025, moments_theta_step = 0.02, baseline = 0.5;
    std::array<double, 3> sigma_floor{ { 0.01, 0.01, 0.01 } }, sigma_cap{ { 1.0, 1.0, 1.0 } };
    double xy_merge = 0.5, theta_merge = 0.5;
    int max_components = 8;
    std::array<double, 3> sigma{ { 0.1, 0.1, 0.05 } };
    bool pruned = true;
    int block = 8;
  };
  // Global localisation in one call, host composition only: the sharded search; refinePoses and poseMoments with this
  // rank's scanner (replicated on every rank: at most 1024 lattices, identical inputs on identical devices);
  // mixtureFromHits and mixtureApplyMoments; initWithMixture.  Returns the components.
  std::vector<MixtureComponent> localize(PlanarScanner& scanner, std::shared_ptr<PlanarData> data, int headings,
                                         int cell_stride, int k, const LocalizeSettings& s)
  {
    const std::vector<bpf_pose_hit> hits = s.pruned ? searchPosesPruned(data, headings, cell_stride, k, s.block)
                                                    : searchPoses(data, headings, cell_stride, k);
    const std::vector<bpf_pose_refined> refined = scanner.refinePoses(
        data, hits, s.refine_xy_radius, s.refine_xy_step, s.refine_theta_radius, s.refine_theta_step, s.refine_levels);
    const std::vector<bpf_pose_moments> rows = scanner.poseMoments(
        data, refined, s.moments_xy_radius, s.moments_xy_step, s.moments_theta_radius, s.moments_theta_step, s.baseline);
    PoseMixture mix = mixtureFromHits(refined, pf_->maxSamples(), s.xy_merge, s.theta_merge, s.max_components, s.sigma);
    mix.mixtureApplyMoments(rows, s.sigma_floor, s.sigma_cap);
    initWithMixture(mix.components);
    return mix.components;
  }
  // BPF_SHARD_RESAMPLE_WINDOW (the default) or BPF_SHARD_RESAMPLE_IN_PLACE: the systematic resampler resamples this
  // rank's slice into itself (badger_pf.h, bpf_shard_set_resample_form); every rank sets the same values
  void setResampleForm(int form, double max_share = 2.0)
  {
    e().check(bpf_shard_set_resample_form(e().get(), form, max_share));
  }
  // BPF_SHARD_RESAMPLE_WINDOW (the default) or BPF_SHARD_RESAMPLE_IN_PLACE: the MULTINOMIAL resampler resamples this
  // rank's slice into itself, the stop index from the ranks' bin lists (badger_pf.h, bpf_shard_set_multinomial_form);
  // max_share and the rebalance setting apply to it as to the systematic form; every rank sets the same value
  void setMultinomialForm(int form)
  {
    e().check(bpf_shard_set_multinomial_form(e().get(), form));
  }
  // BPF_SHARD_REBALANCE_OFF (the default) or BPF_SHARD_REBALANCE_AUTO: an in-place resample never falls back to the
  // window form, and slices more uneven than trigger_share * ceil(M / W) -- a policy condition -- go back to the even
  // split behind it (badger_pf.h, bpf_shard_set_rebalance); every rank sets the same values
  void setRebalance(int mode, double trigger_share = 1.5)
  {
    e().check(bpf_shard_set_rebalance(e().get(), mode, trigger_share));
  }
  // The slices back to the even split in global order; only the samples on the wrong rank move (one ragged gather of
  // their x / y / theta / w bits).  Returns the samples moved over all ranks, the same on every rank; 0: the split was
  // even already.  The totals of a sensor update are dropped: not between updateSensor and updateResample.
  long long rebalance()
  {
    long long moved = 0;
    moved_ = 0;
    e().check(bpf_shard_rebalance(e().get(), &moved));
    e().check(bpf_shard_slice(e().get(), &global_first_, &local_count_, &form_used_));
    moved_ = moved;
    return moved;
  }
  // ParticleFilter::updateResample over the shards; this rank adopts its even share of the new set, or -- in place --
  // keeps the teeth of its own slice: where the slice sits afterwards is the engine's record
  // With BPF_SHARD_REBALANCE_AUTO the call can fail AFTER its resample became current, in the rebalance behind it
  // (bpf_shard_resample_committed): the figures below then describe the new, uneven set before the error is thrown,
  // resampleCommitted() tells, and the caller must not resample again (rebalance() is the step that is left).
  void updateResample()
  {
    const int rc = bpf_shard_update_resample(e().get(), &global_count_, &leaf_count_, &bin_count_, &windows_,
                                             &window_hint_, &cdf_miss_);
    const std::string why = rc == BPF_OK ? std::string() : std::string(bpf_last_error_message(e().get()));
    int committed = 0;
    bpf_shard_resample_committed(e().get(), &committed);
    committed_ = committed != 0;
    moved_ = 0;
    if (rc == BPF_OK || committed_)
      e().check(bpf_shard_slice(e().get(), &global_first_, &local_count_, &form_used_));
    if (rc != BPF_OK)
      throw std::runtime_error("bpf: " + why + " (" + bpf_error_string(rc) + ")");
    int mode = BPF_SHARD_REBALANCE_OFF;
    double share = 0.0;
    e().check(bpf_shard_get_rebalance(e().get(), &mode, &share));
    if (mode == BPF_SHARD_REBALANCE_AUTO && form_used_ == BPF_SHARD_RESAMPLE_IN_PLACE)
      e().check(bpf_shard_rebalance_last(e().get(), &moved_));
  }
  // Node2D::getMaxWeightPose over the GLOBAL set, the same bits on every rank
  void getMaxWeightPose(double* max_weight_out, std::array<double, 3>* max_pose)
  {
    double pose[3] = { 0, 0, 0 };
    e().check(bpf_shard_get_max_weight_pose(e().get(), max_weight_out, pose));
    *max_pose = { pose[0], pose[1], pose[2] };
  }
  // Node::publishParticleCloud's poses of the GLOBAL set in global order (samples first, first + stride, ...), on rank
  // `root` or, with root = -1, on every rank: *poses7 ends as count x 7 doubles there and empty elsewhere (where it may
  // be null).  Returns whether this rank received the array.
  bool getPoseArray(int root, std::vector<double>* poses7, long long first = 0, int stride = 1)
  {
    const bool receives = root < 0 || root == rank_;
    const long long n = global_count_;
    const long long room = (stride >= 1 && first >= 0 && first < n) ? (n - first + stride - 1) / stride : 0;
    if (receives && poses7 && poses7->size() < (size_t)(7 * room + 7))
      poses7->resize((size_t)(7 * room + 7));
    int count = 0;
    e().check(bpf_shard_get_pose_array(e().get(), root, first, stride, receives && poses7 ? poses7->data() : nullptr,
                                       (int)room, &count));
    if (poses7)
      poses7->resize(receives ? (size_t)7 * (size_t)count : 0);
    return receives;
  }
  // ParticleFilter::getClusterStats over the GLOBAL set
  bool getClusterStats(int cidx, double* weight, std::array<double, 3>* mean)
  {
    int count = 0;
    e().check(bpf_shard_compute_cluster_stats(e().get(), &count, nullptr, nullptr, &route_));
    return pf_->getClusterStats(cidx, weight, mean);
  }
  // instead of bootstrap(): this rank's engine was connected from outside (bpf_shard_connect_local)
  void joined(int rank, int world)
  {
    rank_ = rank;
    world_ = world;
  }
  void shutdown() { e().check(bpf_shard_shutdown(e().get())); }
  ParticleFilter& filter() { return *pf_; }
  int globalSampleCount() const { return global_count_; }
  int leafCount() const { return leaf_count_; }
  int binCount() const { return bin_count_; }
  int windowsUsed() const { return windows_; }
  bool cdfMiss() const { return cdf_miss_ != 0; }
  int statsRoute() const { return route_; }  // BPF_SHARD_STATS_ROUTE_* of the last getClusterStats
  int treeRoute() const { return tree_route_; }  // BPF_SHARD_TREE_ROUTE_* of the last init
  long long globalFirst() const { return global_first_; }
  int localCount() const { return local_count_; }  // samples of this rank's slice after the last resample
  int formUsed() const { return form_used_; }      // BPF_SHARD_RESAMPLE_* of the last resample
  long long rebalanced() const { return moved_; }  // samples the last rebalance() / AUTO resample moved over all ranks
  bool resampleCommitted() const { return committed_; }  // the last updateResample made its new set current
  int rank() const { return rank_; }
  int world() const { return world_; }

private:
  Engine& e() { return pf_->engine(); }
  // first global index of this rank's even share of n samples: the split the resample leaves
  long long evenFirst(long long n) const { return n * rank_ / world_; }
  void afterInit()
  {
    global_count_ = pf_->maxSamples();
    global_first_ = evenFirst(global_count_);
    e().check(bpf_shard_global_leaf_count(e().get(), &leaf_count_, &bin_count_));  // in force: no exchange
    e().check(bpf_shard_tree_last_route(e().get(), &tree_route_));
    window_hint_ = first_window_;
    windows_ = cdf_miss_ = 0;
  }
  std::shared_ptr<ParticleFilter> pf_;
  int global_count_, leaf_count_, window_hint_, first_window_;
  long long global_first_;
  int bin_count_ = 0, windows_ = 0, cdf_miss_ = 0, route_ = 0, tree_route_ = 0;
  int local_count_ = 0, form_used_ = BPF_SHARD_RESAMPLE_WINDOW;
  long long moved_ = 0;
  bool committed_ = false;
  int rank_ = 0, world_ = 1;
};

// The same filter with ALL its ranks in this process -- a single-process node with several engines (badger_pf.h,
// bpf_shard_connect_local).  Owns the W rank filters and W worker threads, one per engine; every member below fans
// out to the workers, each of which makes the collective call for its rank (the ranks meet inside the library at the
// exchanges), and joins them.  Same member names as ShardedParticleFilter.  When some ranks fail and others do not it
// throws "the ranks' statuses differ"; when all fail, rank 0's error; otherwise it returns rank 0's figures.  The
// object itself is driven from one thread.
class LocalShardedParticleFilter
{
public:
  // pfs[r]: rank r's filter on an engine of its own, created with the GLOBAL min / max sample counts.  counts[r]:
  // samples of the slice loaded into it by hand (leaf_count: of the whole set's tree, as for ShardedParticleFilter);
  // empty when initWithGaussian / initWithRandomPoses follows.
  explicit LocalShardedParticleFilter(std::vector<std::shared_ptr<ParticleFilter>> pfs, std::vector<int> counts = {},
                                      int leaf_count = 1, int first_window = 4096)
  {
    const int W = (int)pfs.size();
    if (W < 1 || (!counts.empty() && (int)counts.size() != W))
      throw std::invalid_argument("LocalShardedParticleFilter: one filter (and one count) per rank");
    std::vector<bpf_engine*> engines;
    for (auto& p : pfs)
      engines.push_back(p->engine().get());
    const int rc = bpf_shard_connect_local(engines.data(), W, 0);
    if (rc != BPF_OK)
      throw std::runtime_error(std::string("bpf_shard_connect_local: ") + bpf_error_string(rc));
    long long total = 0, first = 0;
    for (int c : counts)
      total += c;
    for (int r = 0; r < W; ++r)
    {
      ranks_.emplace_back(new ShardedParticleFilter(pfs[(size_t)r], (int)total, leaf_count, first_window, first));
      ranks_.back()->joined(r, W);
      first += counts.empty() ? 0 : counts[(size_t)r];
    }
    workers_.resize((size_t)W);
    for (int r = 0; r < W; ++r)
      workers_[(size_t)r].thread = std::thread([this, r] { work(r); });
  }
  ~LocalShardedParticleFilter()
  {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    wake_.notify_all();
    for (auto& w : workers_)
      w.thread.join();
  }
  LocalShardedParticleFilter(const LocalShardedParticleFilter&) = delete;
  LocalShardedParticleFilter& operator=(const LocalShardedParticleFilter&) = delete;

  // fn(rank, filter of that rank) on every rank's thread at once: map / scanner / model set-up, dumps
  void forEachRank(const std::function<void(int, ParticleFilter&)>& fn)
  {
    fanOut([&](int r) { fn(r, ranks_[(size_t)r]->filter()); });
  }
  void initWithGaussian(const std::array<double, 3>& mean, const std::array<double, 9>& rotation,
                        const std::array<double, 3>& sigma)
  {
    fanOut([&](int r) { ranks_[(size_t)r]->initWithGaussian(mean, rotation, sigma); });
  }
  void initWithRandomPoses()
  {
    fanOut([&](int r) { ranks_[(size_t)r]->initWithRandomPoses(); });
  }
  void initWithMixture(const std::vector<MixtureComponent>& components)
  {
    fanOut([&](int r) { ranks_[(size_t)r]->initWithMixture(components); });
  }
  bool updateAction(std::shared_ptr<OdomData> data)
  {
    fanOut([&](int r) { ranks_[(size_t)r]->updateAction(data); });
    return true;
  }
  bool updateSensor(std::shared_ptr<PlanarData> data)
  {
    fanOut([&](int r) { ranks_[(size_t)r]->updateSensor(data); });
    return true;
  }
  bool updateSensorCloud(const float* xyz, int n)
  {
    fanOut([&](int r) { ranks_[(size_t)r]->updateSensorCloud(xyz, n); });
    return true;
  }
  // the sharded searches and localize() of every rank; the ranks' rows are compared as bytes, rank 0's come back.
  // stats_out, when given, receives every rank's counters
  std::vector<bpf_pose_hit> searchPoses(std::shared_ptr<PlanarData> data, int headings, int cell_stride, int k,
                                        long long first = 0, long long count = -1)
  {
    return sameRows([&](int r) { return ranks_[(size_t)r]->searchPoses(data, headings, cell_stride, k, first, count); });
  }
  std::vector<bpf_pose_hit> searchPosesPruned(std::shared_ptr<PlanarData> data, int headings, int cell_stride, int k,
                                              int block = 8, int first_block = 0, int block_count = -1,
                                              std::vector<bpf_pose_search_stats>* stats_out = nullptr)
  {
    std::vector<bpf_pose_search_stats> st(ranks_.size());
    auto rows = sameRows([&](int r) {
      return ranks_[(size_t)r]->searchPosesPruned(data, headings, cell_stride, k, block, first_block, block_count,
                                                  &st[(size_t)r]);
    });
    if (stats_out)
      *stats_out = st;
    return rows;
  }
  std::vector<bpf_pose_hit> searchPosesCloud(const float* xyz, int n_points, int headings, int cell_stride, int k,
                                             long long first = 0, long long count = -1)
  {
    return sameRows(
        [&](int r) { return ranks_[(size_t)r]->searchPosesCloud(xyz, n_points, headings, cell_stride, k, first, count); });
  }
  std::vector<bpf_pose_hit> searchPosesCloudPruned(const float* xyz, int n_points, int headings, int cell_stride,
                                                   int k, int block = 8, int first_block = 0, int block_count = -1,
                                                   std::vector<bpf_pose_search_stats>* stats_out = nullptr)
  {
    std::vector<bpf_pose_search_stats> st(ranks_.size());
    auto rows = sameRows([&](int r) {
      return ranks_[(size_t)r]->searchPosesCloudPruned(xyz, n_points, headings, cell_stride, k, block, first_block,
                                                       block_count, &st[(size_t)r]);
    });
    if (stats_out)
      *stats_out = st;
    return rows;
  }
  // scanners[r]: rank r's scanner
  std::vector<MixtureComponent> localize(const std::vector<std::shared_ptr<PlanarScanner>>& scanners,
                                         std::shared_ptr<PlanarData> data, int headings, int cell_stride, int k,
                                         const ShardedParticleFilter::LocalizeSettings& s)
  {
    if (scanners.size() != ranks_.size())
      throw std::invalid_argument("LocalShardedParticleFilter::localize: one scanner per rank");
    std::vector<std::vector<MixtureComponent>> got(ranks_.size());
    fanOut([&](int r) {
      got[(size_t)r] = ranks_[(size_t)r]->localize(*scanners[(size_t)r], data, headings, cell_stride, k, s);
    });
    for (auto& g : got)
      if (g.size() != got[0].size() ||
          (!g.empty() && std::memcmp(g.data(), got[0].data(), g.size() * sizeof(MixtureComponent)) != 0))
        throw std::runtime_error("LocalShardedParticleFilter: the ranks' mixtures differ");
    return got[0];
  }
  void setResampleForm(int form, double max_share = 2.0)
  {
    for (auto& s : ranks_)
      s->setResampleForm(form, max_share);
  }
  void setMultinomialForm(int form)
  {
    for (auto& s : ranks_)
      s->setMultinomialForm(form);
  }
  void setRebalance(int mode, double trigger_share = 1.5)
  {
    for (auto& s : ranks_)
      s->setRebalance(mode, trigger_share);
  }
  long long rebalance()
  {
    fanOut([&](int r) { ranks_[(size_t)r]->rebalance(); });
    for (auto& s : ranks_)
      if (s->rebalanced() != ranks_[0]->rebalanced())
        throw std::runtime_error("LocalShardedParticleFilter: the ranks moved different numbers of samples");
    return ranks_[0]->rebalanced();
  }
  void updateResample()
  {
    fanOut([&](int r) { ranks_[(size_t)r]->updateResample(); });
    for (auto& s : ranks_)
      if (s->globalSampleCount() != ranks_[0]->globalSampleCount() || s->leafCount() != ranks_[0]->leafCount() ||
          s->binCount() != ranks_[0]->binCount() || s->formUsed() != ranks_[0]->formUsed())
        throw std::runtime_error("LocalShardedParticleFilter: the ranks resampled to different sets");
  }
  void getMaxWeightPose(double* max_weight_out, std::array<double, 3>* max_pose)
  {
    std::vector<double> w(ranks_.size());
    std::vector<std::array<double, 3>> p(ranks_.size());
    fanOut([&](int r) { ranks_[(size_t)r]->getMaxWeightPose(&w[(size_t)r], &p[(size_t)r]); });
    *max_weight_out = w[0];
    *max_pose = p[0];
  }
  bool getClusterStats(int cidx, double* weight, std::array<double, 3>* mean)
  {
    std::vector<double> w(ranks_.size());
    std::vector<std::array<double, 3>> m(ranks_.size());
    std::vector<char> ok(ranks_.size());
    fanOut([&](int r) { ok[(size_t)r] = ranks_[(size_t)r]->getClusterStats(cidx, &w[(size_t)r], &m[(size_t)r]); });
    if (ok[0])
    {
      *weight = w[0];
      *mean = m[0];
    }
    return ok[0] != 0;
  }
  // Node::publishParticleCloud's poses of the GLOBAL set, received by rank 0's engine
  bool getPoseArray(std::vector<double>* poses7, long long first = 0, int stride = 1)
  {
    fanOut([&](int r) { ranks_[(size_t)r]->getPoseArray(0, r == 0 ? poses7 : nullptr, first, stride); });
    return true;
  }
  void shutdown()
  {
    for (auto& s : ranks_)
      s->shutdown();
  }
  ShardedParticleFilter& rank(int r) { return *ranks_[(size_t)r]; }
  int world() const { return (int)ranks_.size(); }
  int globalSampleCount() const { return ranks_[0]->globalSampleCount(); }
  int leafCount() const { return ranks_[0]->leafCount(); }
  int binCount() const { return ranks_[0]->binCount(); }
  int windowsUsed() const { return ranks_[0]->windowsUsed(); }
  int formUsed() const { return ranks_[0]->formUsed(); }
  long long rebalanced() const { return ranks_[0]->rebalanced(); }
  int statsRoute() const { return ranks_[0]->statsRoute(); }
  bool cdfMiss() const
  {
    for (auto& s : ranks_)
      if (s->cdfMiss())
        return true;
    return false;
  }

private:
  struct Worker
  {
    std::thread thread;
    bool has_job = false;
    std::exception_ptr error;
  };
  void work(int r)
  {
    std::unique_lock<std::mutex> lk(m_);
    for (;;)
    {
      wake_.wait(lk, [&] { return stop_ || workers_[(size_t)r].has_job; });
      if (stop_)
        return;
      lk.unlock();
      std::exception_ptr err;
      try
      {
        job_(r);
      }
      catch (...)
      {
        err = std::current_exception();
      }
      lk.lock();
      workers_[(size_t)r].error = err;
      workers_[(size_t)r].has_job = false;
      if (--pending_ == 0)
        done_.notify_all();
    }
  }
  void fanOut(const std::function<void(int)>& fn)
  {
    std::unique_lock<std::mutex> lk(m_);
    job_ = fn;
    pending_ = (int)workers_.size();
    for (auto& w : workers_)
    {
      w.has_job = true;
      w.error = nullptr;
    }
    wake_.notify_all();
    done_.wait(lk, [&] { return pending_ == 0; });
    int failed = 0;
    for (auto& w : workers_)
      failed += w.error ? 1 : 0;
    if (failed == 0)
      return;
    if (failed != (int)workers_.size())
      throw std::runtime_error("LocalShardedParticleFilter: the ranks' statuses differ (" + std::to_string(failed) +
                               " of " + std::to_string(workers_.size()) + " failed)");
    std::rethrow_exception(workers_[0].error);
  }
  // search(rank) on every rank's thread; rank 0's rows after all ranks' rows were compared as bytes
  std::vector<bpf_pose_hit> sameRows(const std::function<std::vector<bpf_pose_hit>(int)>& search)
  {
    std::vector<std::vector<bpf_pose_hit>> got(ranks_.size());
    fanOut([&](int r) { got[(size_t)r] = search(r); });
    for (auto& g : got)
      if (g.size() != got[0].size() ||
          (!g.empty() && std::memcmp(g.data(), got[0].data(), g.size() * sizeof(bpf_pose_hit)) != 0))
        throw std::runtime_error("LocalShardedParticleFilter: the ranks' search rows differ");
    return got[0];
  }
  std::vector<std::unique_ptr<ShardedParticleFilter>> ranks_;
  std::vector<Worker> workers_;
  std::mutex m_;
  std::condition_variable wake_, done_;
  std::function<void(int)> job_;
  int pending_ = 0;
  bool stop_ = false;
};

}  // namespace badger_amcl_amd
