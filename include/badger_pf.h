/*
 * badger_pf.h -- C-ABI of libbadger_pf_hip.so, the MI355X (gfx950) engine for the
 * badger_amcl sensor-update + resample hot path.
 *
 * Everything here is plain C: opaque handle, pointers and sizes, int status codes.
 * No exception, C++ type or torch type crosses this boundary.  One engine is used
 * by one host thread at a time (the reference's seams are single-caller too:
 * SURVEY.md section 8(b), "Threading").
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * the reference checkout).  INTEGRATION.md shows the C++ binding a maintainer of
 * the reference would add on top of this header.
 *
 * Memory conventions
 *   "samples" buffers are the reference's PFSample array seen as doubles: AoS
 *   {x, y, theta, weight}, 32 bytes per particle (include/amcl/pf/particle_filter.h:41-49).
 *   Host pointers are caller-owned and only read/written during the call.
 *   Functions whose name contains `_dev` take DEVICE pointers the caller owns
 *   (e.g. a torch tensor's data_ptr()) and run asynchronously on the engine stream.
 */
#ifndef BADGER_PF_H
#define BADGER_PF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bpf_engine bpf_engine;

/* ---- status codes (the reference has none: it returns 0.0 / false or ROS_ASSERTs;
 * see SURVEY.md 8(b) "Error conventions") */
enum
{
  BPF_OK = 0,
  BPF_ERR_INVALID_ARGUMENT = 1,
  BPF_ERR_NOT_CONFIGURED = 2,     /* map / model / filter missing */
  BPF_ERR_HIP = 3,                /* a HIP runtime call failed; see bpf_last_error_message */
  BPF_ERR_UNSUPPORTED = 4,        /* e.g. w_diff > 0 needs the node's random_pose_fn_ callback */
  BPF_ERR_CDF_MISS = 5,           /* reference ROS_ASSERT(i < sample_count), particle_filter.cpp:399 */
  BPF_ERR_LUT_LEVELS = 6,         /* distance LUT holds more than 8190 distinct values */
  BPF_ERR_BEAM_STEP = 7,          /* beam model with range_count < max_beams: the reference never returns */
  BPF_ERR_CAPACITY = 8,
  BPF_ERR_EXCHANGE = 9            /* mailbox exchange: a peer's word did not arrive within 5 s */
};

enum
{
  BPF_MODEL_BEAM = 0,                       /* PLANAR_MODEL_BEAM */
  BPF_MODEL_LIKELIHOOD_FIELD = 1,           /* PLANAR_MODEL_LIKELIHOOD_FIELD */
  BPF_MODEL_LIKELIHOOD_FIELD_PROB = 2,      /* PLANAR_MODEL_LIKELIHOOD_FIELD_PROB */
  BPF_MODEL_LIKELIHOOD_FIELD_GOMPERTZ = 3   /* PLANAR_MODEL_LIKELIHOOD_FIELD_GOMPERTZ */
};

enum
{
  BPF_RESAMPLE_MULTINOMIAL = 0, /* PF_RESAMPLE_MULTINOMIAL */
  BPF_RESAMPLE_SYSTEMATIC = 1   /* PF_RESAMPLE_SYSTEMATIC */
};

enum
{
  BPF_CLOUD_MODEL = 0,          /* POINT_CLOUD_MODEL */
  BPF_CLOUD_MODEL_GOMPERTZ = 1  /* POINT_CLOUD_MODEL_GOMPERTZ */
};

/* ------------------------------------------------------------------ lifecycle */
int bpf_create(int device_ordinal, bpf_engine** out);
void bpf_destroy(bpf_engine* e);
const char* bpf_error_string(int code);
const char* bpf_last_error_message(const bpf_engine* e);
/* Run the engine's work on a caller-provided hipStream_t.  NULL is HIP's default (null) stream,
 * which is what torch.cuda.current_stream().cuda_stream reports unless a side stream is active;
 * BPF_OWN_STREAM restores the engine's own non-blocking stream. */
#define BPF_OWN_STREAM ((void*)(intptr_t)-1)
int bpf_set_stream(bpf_engine* e, void* hip_stream);
int bpf_synchronize(bpf_engine* e);

/* ------------------------------------------------------------------ 2-D map
 * OccupancyMap state (include/amcl/map/occupancy_map.h:93-102, map.h:48-53):
 * cells = cells_.data() (MapCellState is a 32-bit enum: -1 free, 0 unknown, +1
 * occupied; index i + j*size_x), dist_lut = distances_lut_.data() (may be NULL),
 * origin = origin_.x/.y (float), resolution_, max_distance_to_object_. */
int bpf_map2d_set(bpf_engine* e, const int32_t* cells, const float* dist_lut, int size_x, int size_y,
                  float origin_x, float origin_y, double resolution, double max_dist);
/* The FAST, explicitly named alternative to OccupancyMap::updateDistancesLUT (occupancy_map.cpp:138-160): the exact
 * Euclidean distance capped at max_dist, on the reference's (a,b)-integer lattice, built on the device in
 * milliseconds.  NOT the reference's values: its brushfire is approximate (>= this, equal in > 99 % of the cells).
 * The call that gives the reference's values is bpf_map2d_build_distances_lut_reference below, and that is what the
 * host mirrors' `updateDistancesLUT` and the implicit build of bpf_planar_set_model_likelihood_field* use unless
 * BPF_OPT_LUT_EXACT_EDT is set. */
int bpf_map2d_build_distances_lut(bpf_engine* e, double max_dist);
int bpf_map2d_get_distances_lut(bpf_engine* e, float* out, size_t capacity);
/* OccupancyMap::calcRange(ox, oy, oa, max_range) (occupancy_map.cpp:257-364) for n rays: the integer Bresenham
 * walk from the cell of (ox, oy) towards the cell of the max-range end point, distance to the first cell that is off
 * the map or not FREE (max_range if none; 0 for a start off the map).  The direction comes as cos(oa), sin(oa),
 * formed by the caller as the reference forms them (libm), so that the end cell is the reference's bit for bit.
 * Needs only the cells (bpf_map2d_set); host buffers in and out. */
int bpf_map2d_calc_range(bpf_engine* e, const double* ox, const double* oy, const double* cos_a, const double* sin_a,
                         const double* max_range, int n, double* range_out);
/* OccupancyMap::updateDistancesLUT exactly as the reference builds it (occupancy_map.cpp:138-252):
 * priority-queue brushfire on the host (std::priority_queue, so tie order matches a libstdc++
 * build of the reference), ~0.45 s for a 2000 x 2000 map, once per map as in the reference.  THE DEFAULT behind the
 * reference-named calls. */
int bpf_map2d_build_distances_lut_reference(bpf_engine* e, double max_dist);

/* ------------------------------------------------------------------ caller-owned host buffers
 * The reference keeps its particles in host memory: ParticleFilter allocates `samples` once at max_samples
 * (src/amcl/pf/particle_filter.cpp:62-89, include/amcl/pf/particle_filter.h:70-75) and every sensor model gets that
 * vector (planar_scanner.cpp:141-164).  Registering the buffer (hipHostRegister: pins it and maps it for the copy
 * engines, ~1 ms, once) lets the host-buffer entry points below move it at PCIe rate without a staging copy by the
 * calling thread.  [ptr, ptr + bytes) need not be aligned.  The owner must keep the memory allocated until
 * bpf_host_buffer_unregister (same ptr) or bpf_destroy.  Unregistered buffers work everywhere, through the runtime's
 * bounce buffers.  bpf_host_buffer_is_registered: 1 when the whole range lies inside one registered buffer. */
int bpf_host_buffer_register(bpf_engine* e, void* ptr, size_t bytes);
int bpf_host_buffer_unregister(bpf_engine* e, void* ptr);
int bpf_host_buffer_is_registered(bpf_engine* e, const void* ptr, size_t bytes);
/* 3 when the last likelihood-field scoring launch of a resident set walked the particles in map-tile order
 * (BPF_OPT_TILE_SORT), 0 otherwise */
int bpf_score_last_form(bpf_engine* e, int* form_out);
/* which form the last device-side histogram tree took: 2 = grown in LDS-sized pieces (kernels_kld2.hpp), 1 = one launch
 * pair per level (also after the pieces declined a stream), 3 = the persistent launch, 4 = no tree: the distinct-key
 * count of BPF_KLD_COUNT_BINS (bpf_pf_set_kld_count), 0 = none yet */
int bpf_kld_last_form(bpf_engine* e, int* form_out);
/* which instance of the 3-D scoring kernel the last point-cloud launch of this engine took: 0 = none yet, otherwise
 * 32 | bits with 1 = the exact-reciprocal voxel form (1 / resolution representable), 2 = PLANAR (mounting without roll
 * or pitch), 4 = DENSE (gathers from the dense tiled copy of the LUT), 8 = BORDER (off-map cells read the volume's
 * border ring), 16 = the graded partition of the particles was on.  Read-only: it has no effect on any launch. */
int bpf_cloud_last_form(bpf_engine* e, int* form_out);
/* what the last bpf_planar_apply_model_to_sample_set did: chunks of the pipelined form (0 = the plain upload / score /
 * download sequence, -1 = one scoring launch that read and wrote the registered records in place); pinned = the buffer
 * lies in a registered range */
int bpf_seam_last_plan(bpf_engine* e, int* chunks_out, int* pinned_out);

/* ------------------------------------------------------------------ planar scanner
 * PlanarScanner::{init, setModel*, setMapFactors, setPlanarScannerPose}
 * (include/amcl/sensors/planar_scanner.h:62-93, planar_scanner.cpp:49-121,535-538). */
int bpf_planar_init(bpf_engine* e, int max_beams);
int bpf_planar_set_model_beam(bpf_engine* e, double z_hit, double z_short, double z_max, double z_rand,
                              double sigma_hit, double lambda_short);
int bpf_planar_set_model_likelihood_field(bpf_engine* e, double z_hit, double z_rand, double sigma_hit,
                                          double max_distance_to_object);
int bpf_planar_set_model_likelihood_field_prob(bpf_engine* e, double z_hit, double z_rand, double sigma_hit,
                                               double max_distance_to_object, int do_beamskip,
                                               double beam_skip_distance, double beam_skip_threshold,
                                               double beam_skip_error_threshold);
int bpf_planar_set_model_likelihood_field_gompertz(bpf_engine* e, double z_hit, double z_rand, double sigma_hit,
                                                   double max_distance_to_object, double gompertz_a,
                                                   double gompertz_b, double gompertz_c, double input_shift,
                                                   double input_scale, double output_shift);
int bpf_planar_set_map_factors(bpf_engine* e, double off_map_factor, double non_free_space_factor,
                               double non_free_space_radius);
int bpf_planar_set_scanner_pose(bpf_engine* e, const double pose[3]);

/* Seam A, host buffers: PlanarScanner::applyModelToSampleSet (planar_scanner.cpp:141-164).
 * Multiplies samples[i].weight in place for i < sample_count and returns their sum
 * (0.0 on failure, like the reference); *status (nullable) receives a BPF_* code.
 * ranges/angles/range_count/range_max are PlanarData (planar_scanner.h:45-54);
 * set_converged is PFSampleSet::converged (only the prob model reads it).
 * A registered, 16-byte aligned buffer (bpf_host_buffer_register) of 4 096 records or more under a likelihood-field
 * model is not copied at all: one scoring launch reads the records over PCIe as its waves reach them and writes them
 * back whole with the new weight.  Other sets of 40 k particles or more go through in two chunks
 * (BPF_OPT_SEAM_CHUNKS): chunk k is scored while chunk k + 1 crosses PCIe, the scoring launches store the weights into
 * pinned host memory themselves (no download) and the calling thread writes chunk k's weights into the records while
 * chunk k + 1 is scored.  Same weights bit for bit as the plain upload / score / download sequence. */
double bpf_planar_apply_model_to_sample_set(bpf_engine* e, double* samples, int sample_count, int set_converged,
                                            const double* ranges, const double* angles, int range_count,
                                            double range_max, int* status);

/* ------------------------------------------------------------------ particle filter
 * Device-resident ParticleFilter (include/amcl/pf/particle_filter.h:92-184).  The two
 * ping-pong sample sets live in HBM as structure-of-arrays. */
int bpf_pf_create(bpf_engine* e, int min_samples, int max_samples, double alpha_slow, double alpha_fast,
                  double global_localization_convergence_threshold);  /* ctor, particle_filter.cpp:38-98 */
int bpf_pf_set_resample_model(bpf_engine* e, int resample_model);             /* :100-103 */
int bpf_pf_set_population_size_parameters(bpf_engine* e, double pop_err, double pop_z); /* :651-655 */
int bpf_pf_set_decay_rates(bpf_engine* e, double alpha_slow, double alpha_fast);        /* :657-661 */
/* The reference draws from the process-global drand48 stream (particle_filter.cpp:309,385,393);
 * the engine carries that 48-bit state explicitly so host code can hand it over and take it back. */
int bpf_pf_srand48(bpf_engine* e, long seed);
int bpf_pf_set_rng_state(bpf_engine* e, uint64_t state48);
int bpf_pf_get_rng_state(const bpf_engine* e, uint64_t* state48);
/* Load the current set (what initWithPoseFn/initWithGaussian leave behind, :106-162):
 * resets w_slow/w_fast and converged.  leaf_count = that set's kd-tree leaf count, or -1
 * to have it computed from the poses -- when something first needs it (bpf_pf_get_state, the systematic resampler,
 * a snapshot) or before the poses move (a motion update): the tree is that of the poses handed over here, as in the
 * reference, but a cycle that uploads, updates and resamples with the multinomial resampler never builds it.
 * A registered `samples` buffer (bpf_host_buffer_register) is read by the copy engine directly. */
int bpf_pf_set_samples(bpf_engine* e, const double* samples, int sample_count, int leaf_count);
int bpf_pf_get_samples(bpf_engine* e, double* samples_out, int capacity, int* sample_count_out);
/* Keep a device-resident copy of the current set (poses, weights, counts) and put it back
 * later with one device-to-device copy -- stands in for the motion update, which rewrites
 * every pose of the set each cycle (Odom::updateAction, out of scope here). */
int bpf_pf_snapshot(bpf_engine* e);
int bpf_pf_restore(bpf_engine* e);
/* Overwrite the weights of the current set with one value (bench harness: restores 1/N). */
int bpf_pf_fill_weights(bpf_engine* e, double weight);

/* Seam A on the resident set: PlanarScanner::updateSensor(pf, data)
 * = ParticleFilter::updateSensor(applyModelToSampleSet, data)
 * (planar_scanner.cpp:125-137, particle_filter.cpp:223-267).  Asynchronous. */
int bpf_pf_update_sensor_planar(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                double range_max);
/* random_pose_fn_ of the ParticleFilter constructor (particle_filter.cpp:40-47), used by both resamplers when
 * w_diff = max(0, 1 - w_fast / w_slow) > 0 (augmented-MCL recovery, :295-324 and :383-388).  The node passes
 * Node::uniformPoseGenerator; with its score check disabled (uniform_pose_starting_weight_threshold = 0, the
 * node's default, node.cpp:124,847-868) that is Node::randomFreeSpacePose (node.cpp:823-845): two drand48 draws,
 * a uniformly chosen cell of Node2D::updateFreeSpaceIndices (node_2d.cpp:317-337: FREE and further than
 * non_free_space_radius from an obstacle) and a uniform heading.  BPF_RANDOM_POSE_FREE_SPACE_2D evaluates exactly
 * that on the device from the engine's own 2-D map, drawing from the filter's drand48 stream in the reference's
 * order; with BPF_RANDOM_POSE_NONE (default) a resample that needs random poses returns BPF_ERR_UNSUPPORTED.
 * BPF_RANDOM_POSE_FREE_SPACE_3D is the same over Node3D::updateFreeSpaceIndices (node_3d.cpp:306-318): every
 * (i, j) column with min_cells[0] <= i < max_cells[0] and min_cells[1] <= j < max_cells[1] of bpf_map3d_set, i outer
 * and j inner, placed by OctoMap::convertMapToWorld (octomap.cpp:83-95: x = i * resolution, y = j * resolution, no
 * origin, no half-cell offset).  It needs only the 3-D map.  All three consumers (initWithPoseFn and both
 * resamplers' recovery draws) use the generator set here, with the score check of bpf_pf_set_uniform_pose_check. */
enum
{
  BPF_RANDOM_POSE_NONE = 0,
  BPF_RANDOM_POSE_FREE_SPACE_2D = 1,
  BPF_RANDOM_POSE_FREE_SPACE_3D = 2
};
int bpf_pf_set_random_pose_generator(bpf_engine* e, int mode);
/* The score check of Node::uniformPoseGenerator (node.cpp:847-868), parameters uniform_pose_starting_weight_threshold
 * (g0) and uniform_pose_deweight_multiplier (m) (cfg/AMCL.cfg:35-36, node.cpp:124-125,255-256):
 *     p = randomFreeSpacePose();
 *     if (g0 > 0 && m < 1 && m >= 0)
 *       while (scorePose(p) < good_weight) { p = randomFreeSpacePose(); good_weight *= m; }
 * What the reference's score is: Node2D::scorePose (node_2d.cpp:298-316) copies the member PFSample fake_sample_
 * (node_2d.h:99, a value) into fake_sample_set_->samples, scores that one-sample set and returns
 * fake_sample_.weight, the untouched member: always 1.0, with or without a scan.  Node3D::scorePose does the same
 * (node_3d.cpp:286-304, node_3d.h:105).  The loop is therefore a fixed number of rejected trials per call,
 * K = min{k : !(1.0 < thr[k])} with thr[0] = g0, thr[k + 1] = thr[k] * m (repeated double multiplication), 0 when
 * the check is inactive (a NaN g0 or m included).  A call that starts at stream element p takes its pose from
 * elements p + 2K, p + 2K + 1 and consumes 2 (K + 1) elements; a recovery draw of the multinomial resampler then
 * consumes 2K + 3.
 *   scoring = BPF_POSE_CHECK_AS_REFERENCE (0): the score is 1.0, as the reference computes it.
 *   scoring = BPF_POSE_CHECK_SENSOR_MODEL (1): opt-in score-guided recovery, the parameter's documented meaning
 *             ("a pose with at least this sample weight according to the sensor model"): a trial's score is the
 *             weight of the one-sample set {pose, 1.0} after applyModelToSampleSet with set->converged = 0 (no beam
 *             skipping; recalcWeight iff that weight is > 0, planar_scanner.cpp:141-164) against the last scan given
 *             to bpf_pf_update_sensor_planar (bpf_map2d_set clears it, as the node clears latest_scan_data_,
 *             node_2d.cpp:217; with no scan every score is 1.0 and the result is AS_REFERENCE's).  The trial poses
 *             are scored on the device in windows by the planar scoring kernels; the loop runs over those scores.
 *             Parity-unpinned by construction; an accept decision can differ from a serial evaluation only where a
 *             score lies within the kernels' rounding (<= 1e-9 relative) of its threshold.  Planar models only: with
 *             the cloud scanner configured a call that draws random poses returns BPF_ERR_UNSUPPORTED, and so does
 *             bpf_shard_begin_resample in this mode.
 * The default is g0 = 0 (check inactive).  A call whose stream use would pass 31-bit positions (2 (K + 1) per random
 * pose; 2K + 3 per candidate draw of the multinomial chain, for max_samples + 1 draws) returns BPF_ERR_CAPACITY and
 * leaves the set and the drand48 state untouched; so does every call when K would pass 2^30.  The sharded path
 * (bpf_shard_begin_resample) uses the same K. */
enum
{
  BPF_POSE_CHECK_AS_REFERENCE = 0,
  BPF_POSE_CHECK_SENSOR_MODEL = 1
};
int bpf_pf_set_uniform_pose_check(bpf_engine* e, double starting_weight_threshold, double deweight_multiplier,
                                  int scoring);
/* K of the AS_REFERENCE check above for (g0, m); -1 when it would pass 2^30.  Needs no engine. */
int bpf_uniform_pose_retries(double starting_weight_threshold, double deweight_multiplier);
/* What the KLD stop rule counts as k (particle_filter.cpp:411-417 and :276 call resampleLimit(k)).
 *   BPF_KLD_COUNT_LEAVES (0, default): the reference's k, PFKDTree::getLeafCount -- the childless nodes of the
 *     insertion-ordered histogram tree.  Bit-exact with the reference.
 *   BPF_KLD_COUNT_BINS (1, opt-in): k = the number of distinct histogram keys, key = floor(pose / {0.5 m, 0.5 m,
 *     10 deg}) with theta not normalised, as in Fox's KLD-sampling and upstream AMCL.  Parity unpinned by
 *     construction: no reference run computes it.  Multinomial: after draw m (0-based) the set stops when
 *     m + 1 > resampleLimit(distinct keys among draws 0 .. m).  Systematic: the set size is resampleLimit(distinct
 *     keys of the current set), grown by (1 + w_diff) as before.  The drand48 stream, the draws, the recovery
 *     branch and the uniform pose check are unchanged.  Every leaf count the engine reports or accepts is then a
 *     bin count: bpf_pf_state.leaf_count == bin_count, the leaf_count argument of bpf_pf_set_samples (-1 still
 *     computes it), leaf_count_io of the bpf_shard_* resample calls and the bpf_kld_* stage calls.
 * The mode belongs to the engine, not to a filter: bpf_pf_create does not reset it, so a filter created on an engine
 * switched to BINS counts bins.  A change of mode takes effect at the next resample and marks the current set's count
 * stale, as bpf_pf_set_samples(..., -1) does.  Other values return BPF_ERR_INVALID_ARGUMENT and leave the mode. */
enum
{
  BPF_KLD_COUNT_LEAVES = 0,
  BPF_KLD_COUNT_BINS = 1
};
int bpf_pf_set_kld_count(bpf_engine* e, int mode);
int bpf_pf_get_kld_count(const bpf_engine* e, int* mode_out);
/* Seam B: ParticleFilter::updateResample (particle_filter.cpp:423-471). */
int bpf_pf_update_resample(bpf_engine* e);

/* Engine options.  BPF_OPT_CDF_SERIAL = 1 builds the resampling CDF with the reference's
 * serial running sum (one lane, bit-exact, slow) instead of the parallel scan;
 * BPF_OPT_COUNT_CELLS = 1 makes the beam-model kernel count the cells its rays visit. */
enum
{
  BPF_OPT_CDF_SERIAL = 0,
  BPF_OPT_COUNT_CELLS = 1,
  BPF_OPT_WINDOW_PATH = 2,  /* default 0: 1 allows the LDS-window scoring kernels (device-side switch) */
  BPF_OPT_KLD_DEVICE_MIN = 3, /* default 8192: candidate draws left after the first window from which the KLD stop
                               * rule (ordered kd-tree replay) runs on the device instead of the host; 0 = never */
  BPF_OPT_GRADED_SHARES = 4,  /* default 1: the scoring kernel's waves own particle shares graded by the placement
                               * round of their block; 0 = equal shares.  Results do not
                               * depend on it beyond the summation order of the weight total. */
  BPF_OPT_CLOUD_DENSE = 6,    /* default 1: the 3-D scoring kernel gathers from a dense tiled copy of the LUT when the
                               * map allows one (a z plane below 16 MiB, the volume below 1 GiB); 0 = the reference's
                               * two-level layout.  Same results. */
  BPF_OPT_STATS_HOST = 7,     /* default 0: cluster statistics on the device (order-independent fixed-point sums: equal to
                               * the reference's up to summation rounding); 1 = on the host from a copy of the set, in
                               * the reference's serial order, bit for bit */
  BPF_OPT_LUT_HOST = 8,       /* default 0: bpf_map3d_build_distances_lut replays the reference's FIFO brushfire on the device,
                               * generation by generation (same bytes, same column order); 1 = the serial host builder */
  BPF_OPT_KLD_PERSISTENT = 9, /* default 0: one launch pair per level of the device-side histogram tree of a long draw
                               * stream; 1: ONE launch with grid barriers between the levels when the stream fits one
                               * resident round of blocks (measured slower: 0.98 against 0.83 ms per step of the spread
                               * cloud -- every level is ~9 dependent round trips through the Infinity Cache either way) */
  BPF_OPT_LUT_EXACT_EDT = 10, /* default 0: the implicit LUT build of bpf_planar_set_model_likelihood_field* (the reference calls
                               * map_->updateDistancesLUT there, planar_scanner.cpp:74,91,112) is the reference's
                               * brushfire on the host; 1 = the exact EDT on the device (milliseconds, values differ from
                               * the reference's in < 1 % of the cells) */
  BPF_OPT_HOST_AUTO_REGISTER = 11, /* default 0.  1 = the CALLER'S PROMISE that every host buffer of 64 KB or more it hands to
                               * bpf_planar_apply_model_to_sample_set / bpf_pf_set_samples / bpf_pf_get_samples stays
                               * allocated until bpf_destroy: the engine then pins each one on first sight
                               * (hipHostRegister, ~1 ms once) and keeps the registration, keyed by address range.  A
                               * buffer freed or re-allocated under a kept registration makes the next copy fault --
                               * hence off by default; bpf_host_buffer_register is the per-buffer, owner-controlled form */
  BPF_OPT_SEAM_CHUNKS = 12,   /* default 0 = by size and buffer: a registered, 16-byte aligned buffer of 4 096 records or
                               * more is read and written IN PLACE by one scoring launch (no copy); otherwise sets of 40 k
                               * particles or more go up in two chunks; k > 1 forces k chunks (at most 8) of the pipelined
                               * host-buffer seam (bpf_planar_apply_model_to_sample_set); 1 = the plain upload / score /
                               * download sequence.  Same weights either way (bpf_seam_last_plan says which ran). */
  BPF_OPT_KLD_LOCAL = 13,     /* default 1: the device-side histogram tree of a long draw stream is grown in LDS-sized pieces
                               * (one block grows the top from the first 2 048 keys, the later keys are routed through it
                               * and blocks grow the subtrees below its nodes: kernels_kld2.hpp) instead of one launch
                               * pair per level; 0 = the level loop.  Same tree. */
  BPF_OPT_TILE_SORT = 14,     /* default 1: a cloud the previous resample found spread (no KLD stop) or that was just drawn
                               * uniformly is scored in map-tile order, each XCD taking a contiguous eighth of it, when the
                               * map's LUT does not fit an XCD's L2 (tile-sorted scoring); 0 = index
                               * order always.  Same weights. */
  BPF_OPT_HOST_DIRECT_PAGEABLE = 15, /* default 0: pageable host memory (unregistered sample buffers, map and cloud arrays)
                               * goes up through the engine's own pinned bounce buffer, one host copy.  1 = it is handed
                               * to the HIP runtime as it is (faster by that copy), which pins ranges of more than a
                               * megabyte on the fly and KEEPS such pins, keyed by address and size: the caller's
                               * promise that no buffer it passes is ever freed and allocated again at the same address
                               * while the engine lives (a stale pin reads old pages or faults).  Registered buffers
                               * (bpf_host_buffer_register) are always direct. */
  BPF_OPT_FUSED_LDS_TREE = 16, /* default 0: the single-block resample grows a histogram tree of at most 64 keys in wave 0's
                               * registers (cross-lane ballots, no LDS traffic inside the level loop); 1 = the LDS form
                               * with atomics (a reference for tests).  Same tree, same results. */
  BPF_OPT_STAGE_ON_HOST = 17, /* default 0: for the usual scan (every decimated beam shorter than range_max and than
                               * 2^28 cells, no beam skipping mask) the host hands the decimated ranges over and the
                               * scoring's prep launch forms the beams' end points; 1 = the host forms them always,
                               * as it does for every other scan.  Same bits either way.  (BPF_STAGE_ON_HOST set in
                               * the environment makes 1 the value an engine starts with: A/B runs of tools that set
                               * no options.) */
  BPF_OPT_FUSED_RESAMPLE = 5  /* default 1: normalisation + CDF in one launch, and a resample whose candidate stream
                               * fits 4096 draws as one single-block launch (draws, KLD stop rule, weights,
                               * updateConverged); 0 = the separate launches with the host's ordered replay.
                               * Same results either way. */
};
int bpf_set_option(bpf_engine* e, int option, int value);
/* cells visited by calcRange walks since the last reset (BPF_OPT_COUNT_CELLS) */
int bpf_get_cells_walked(bpf_engine* e, unsigned long long* out, int reset);

typedef struct
{
  int sample_count;       /* PFSampleSet::sample_count of the current set */
  int leaf_count;         /* its kd-tree leaf count (PFKDTree::getLeafCount) */
  int bin_count;          /* distinct occupied histogram bins (kd-tree node count) */
  int converged;          /* ParticleFilter::isConverged */
  float percent_converged;
  double total;           /* last sensor_fn total (particle_filter.cpp:235) */
  double w_slow, w_fast;
  double w_diff;          /* of the last updateResample */
  int last_status;        /* BPF_* of the last update_sensor / update_resample */
  int resample_windows;   /* candidate-draw windows used by the last multinomial resample */
  long long evals;        /* particle-beam evaluations of the last sensor update */
  int kld_on_device;      /* where the last resample's histogram tree was grown: 0 host (ordered replay), 1 device,
                           * level-synchronous in HBM (long streams), 2 device, inside the one-block resample kernel */
  int reserved;
} bpf_pf_state;
int bpf_pf_get_state(bpf_engine* e, bpf_pf_state* out);

/* ------------------------------------------------------------------ motion update
 * Odom::setModel / Odom::updateAction (src/amcl/sensors/odom.cpp:63-301, caller node.cpp:1053-1091)
 * on the resident set: 3 PDFGaussian::draw (pdf_gaussian.cpp:77-97) per particle from the filter's
 * drand48 stream, consumed in the reference's order (particle by particle, rejected attempts and
 * r == 0 re-draws included), so the state left for the resampler is exact.  Poses agree with a
 * libm build of the reference to a few ulp (device log / sin / cos). */
enum
{
  BPF_ODOM_MODEL_DIFF = 0,            /* OdomModelType, include/amcl/sensors/odom.h:33-40 */
  BPF_ODOM_MODEL_OMNI = 1,
  BPF_ODOM_MODEL_DIFF_CORRECTED = 2,
  BPF_ODOM_MODEL_OMNI_CORRECTED = 3,
  BPF_ODOM_MODEL_GAUSSIAN = 4
};
int bpf_odom_set_model(bpf_engine* e, int model_type, double alpha1, double alpha2, double alpha3,
                       double alpha4, double alpha5);
/* OdomData: pose, delta, absolute_motion (odom.h:43-52) */
int bpf_pf_update_action(bpf_engine* e, const double pose[3], const double delta[3],
                         const double absolute_motion[3]);
/* the same for one shard of a filter spread over several engines: this engine holds particles
 * [global_first, global_first + local count) of global_count; every rank passes the same rng state
 * (bpf_pf_set_rng_state) and ends with the same one. */
int bpf_shard_update_action(bpf_engine* e, const double pose[3], const double delta[3],
                            const double absolute_motion[3], long long global_first, long long global_count);

/* Initialisers on the resident set, drawing from the filter's drand48 stream like the reference:
 * ParticleFilter::initWithGaussian (particle_filter.cpp:105-132) given what PDFGaussian's constructor derives from
 * the covariance with Eigen::EigenSolver (third party; pdf_gaussian.cpp:32-46,100-131): `rotation` = cr_ (row-major
 * 3x3), `sigma` = cd_ (square roots of the eigenvalues); every sample is mean + cr * (draw(cd0), draw(cd1), draw(cd2)).
 * ParticleFilter::initWithPoseFn (:135-163) with the generator set by bpf_pf_set_random_pose_generator (global
 * localisation, node.cpp:870-882).  Both fill max_samples particles with weight 1/max_samples, build the set's
 * histogram tree (leaf count), zero w_slow / w_fast and clear the converged flag. */
int bpf_pf_init_with_gaussian(bpf_engine* e, const double mean[3], const double rotation[9], const double sigma[3]);
int bpf_pf_init_with_random_poses(bpf_engine* e);

/* Mixture initialiser: the set of K Gaussian components, e.g. the refined hits of a pose search turned into
 * components by bpf_pose_mixture_from_hits.  Not a reference call for K > 1; K = 1 is bpf_pf_init_with_gaussian.
 * The current set becomes what the reference produces by running the body of initWithGaussian's loop
 * (particle_filter.cpp:112-125, pdf_gaussian.cpp:52-70) over the components in index order: component k takes
 * count_k consecutive samples, each mean_k + cr_k * (draw(cd_k[0]), draw(cd_k[1]), draw(cd_k[2])), all components
 * drawing from the ONE drand48 stream of the filter in sample order.  Weight 1 / max_samples; afterwards the
 * histogram tree of the whole set, w_slow = w_fast = 0, converged cleared and the rng advanced by what the whole set
 * consumed, as after bpf_pf_init_with_gaussian.  A component with count 0 is skipped and its other fields are not
 * read.  sigma may be 0 (the draw still consumes its uniforms).
 * BPF_ERR_INVALID_ARGUMENT, with the set, rng and counts as they were and nothing launched: e or comps NULL,
 * n_components outside [1, 1024], a negative count, counts that do not sum to max_samples, a non-finite mean,
 * rotation or sigma of a component that has samples.  BPF_ERR_NOT_CONFIGURED without bpf_pf_create.
 * On the device: one upload of the component table with the prefix of the counts (at most 128 KB), the Gaussian
 * generation of the motion update with the draw's argument looked up per sample, one kernel that forms the poses,
 * one read-back of the generation's result words, then the tree. */
typedef struct
{
  double mean[3];     /* x, y, theta */
  double rotation[9]; /* cr_, row-major, as bpf_pf_init_with_gaussian takes it */
  double sigma[3];    /* cd_ */
  int count;          /* samples drawn from this component, >= 0 */
  int reserved;       /* 0 */
} bpf_mixture_component; /* 128 bytes in every binding */

int bpf_pf_init_with_mixture(bpf_engine* e, const bpf_mixture_component* comps, int n_components);

/* ------------------------------------------------------------------ cluster statistics
 * ParticleFilter::computeClusterStatsForSet (particle_filter.cpp:505-636) with PFKDTree::cluster
 * (pf_kdtree.cpp:58-90,169-194), and what Node2D::getMaxWeightPose (node_2d.cpp:588-617) reads.
 * Evaluated lazily (first query after the set changed) on the device: occupied bins by hash table, clusters by
 * union-find over the bins' 26-neighbourhoods, labels in the reference's creation order, per-cluster sums as
 * order-independent 128-bit fixed-point accumulators (equal to the reference's serial sums up to summation rounding,
 * the same bits every run); the host reads back one small result block, the cluster array only on
 * bpf_pf_get_cluster.  BPF_OPT_STATS_HOST = 1 evaluates on the host from a copy of the set instead, bit for bit in the
 * reference's order. */
typedef struct
{
  int count;        /* PFCluster::count */
  double weight;    /* PFCluster::weight */
  double mean[3];   /* PFCluster::mean */
  double cov[5];    /* PFCluster::cov at (0,0) (0,1) (1,0) (1,1) (2,2); the other entries are unset in the reference */
} bpf_cluster;
/* cluster_count = PFSampleSet::cluster_count; set_mean / set_cov (nullable) = PFSampleSet::mean / cov */
int bpf_pf_compute_cluster_stats(bpf_engine* e, int* cluster_count_out, double set_mean[3], double set_cov[5]);
/* ParticleFilter::getClusterStats(cidx, &weight, &mean): returns BPF_ERR_INVALID_ARGUMENT for cidx >= cluster_count */
int bpf_pf_get_cluster(bpf_engine* e, int cidx, bpf_cluster* out);
/* Node2D::getMaxWeightPose: the heaviest cluster's weight and mean (weight 0 when there is none) */
int bpf_pf_get_max_weight_pose(bpf_engine* e, double* max_weight, double pose[3]);

/* ------------------------------------------------------------------ 3-D map + point cloud
 * OctoMap LUT state (include/amcl/map/octomap.h:96-110): pose_indices_, distance_ratios_,
 * cropped_min_cells_, cropped_max_cells_, resolution_, max_distance_to_object_.
 * Besides the two arrays the engine keeps a dense copy laid out for the scoring kernel's gathers when it fits 1 GiB;
 * this call also reads distance_ratios once on the host to find two byte values no entry holds: they mark the dense
 * copy's border cells (off the map) and one spare plane (a zero term), which is what lets the scoring kernel of a
 * planar mounting do without its on-the-map comparisons.  A LUT that uses more than 254 distinct ratios keeps the
 * comparisons; the weights are the same either way. */
int bpf_map3d_set(bpf_engine* e, const uint32_t* pose_indices, size_t n_pose_indices,
                  const uint8_t* distance_ratios, size_t n_distance_ratios, const int min_cells[3],
                  const int max_cells[3], double resolution, double max_dist);

/* OctoMap::updateDistancesLUT (octomap.cpp:175-333) from the occupied voxel indices instead of an octree
 * (the octomap library is the caller's): `occupied_ijk` = n x (i, j, k) map cells of the occupied leaves in
 * the octree's leaf-iteration order (that order fixes where each z column lands in distance_ratios);
 * min_cells / max_cells = cropped_min_cells_ / cropped_max_cells_.  FIFO brushfire with the reference's uint8
 * quantisation and seeding order (priority_queue<Index3>, octomap.h:49-55), run on the host; the result is
 * uploaded like bpf_map3d_set.  SURVEY 8(f) next-3. */
int bpf_map3d_build_distances_lut(bpf_engine* e, const int* occupied_ijk, size_t n_occupied, const int min_cells[3],
                                  const int max_cells[3], double resolution, double max_dist);
/* copies out what the builder (or bpf_map3d_set) holds; either pointer may be NULL to query the sizes only */
/* FIFO generations the last bpf_map3d_build_distances_lut ran on the device (0: it ran on the host) */
int bpf_map3d_builder_generations(bpf_engine* e, int* generations_out);
int bpf_map3d_get_distances_lut(bpf_engine* e, uint32_t* pose_indices, size_t pose_capacity, size_t* n_pose_indices,
                                uint8_t* distance_ratios, size_t ratios_capacity, size_t* n_distance_ratios);
/* PointCloudScanner::{init, setPointCloudModel, setPointCloudModelGompertz, setMapFactors,
 * setPointCloudScannerToFootprintTF} (point_cloud_scanner.cpp:48-90). */
int bpf_cloud_init(bpf_engine* e, int max_beams);
int bpf_cloud_set_model(bpf_engine* e, double z_hit, double z_rand, double sigma_hit);
int bpf_cloud_set_model_gompertz(bpf_engine* e, double z_hit, double z_rand, double sigma_hit, double gompertz_a,
                                 double gompertz_b, double gompertz_c, double input_shift, double input_scale,
                                 double output_shift);
int bpf_cloud_set_map_factors(bpf_engine* e, double off_map_factor, double non_free_space_factor,
                              double non_free_space_radius);
int bpf_cloud_set_scanner_to_footprint_tf(bpf_engine* e, const double xyz[3], const double quat_xyzw[4]);
/* PointCloudScanner::applyModelToSampleSet (point_cloud_scanner.cpp:106-129); points are
 * PointCloudData::points_ as packed float xyz triples in the scanner frame. */
double bpf_cloud_apply_model_to_sample_set(bpf_engine* e, double* samples, int sample_count, const float* points_xyz,
                                           int n_points, int* status);
/* PointCloudScanner::updateSensor(pf, data) on the resident set (:92-102). */
int bpf_pf_update_sensor_cloud(bpf_engine* e, const float* points_xyz, int n_points);

/* ------------------------------------------------------------------ sharded operation
 * One engine per GPU holds a contiguous shard (rank order = particle index order) of ONE
 * filter.  Scoring needs no exchange; normalisation needs the per-shard weight totals;
 * resampling needs the per-shard CDF sums and one sum-exchange of the candidate draw window.
 * The exchanges themselves (RCCL all-gather / all-reduce over xGMI) are issued by the host
 * layer on the same stream between these stage calls; every `_dev` pointer is device memory
 * and nothing here synchronises with the host.  badger_amcl_amd/sharded.py is the driver. */
/* score + recalcWeight on the local shard; the local weight total lands in scalars[0] */
int bpf_shard_score_planar(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                           double range_max);
/* Beam skipping of the prob model (planar_scanner.cpp:352-395,482-529) needs, per beam, the number of particles
 * of the WHOLE set that agree with it.  When it is active (model prob, do_beamskip, set converged)
 * bpf_shard_score_planar stops after the counting pass and returns BPF_SHARD_NEED_BEAM_COUNTS (> 0, not an error):
 * sum the int32 counts of bpf_shard_beam_counts_dev over the shards in place (all-reduce), then call
 * bpf_shard_score_planar_finish with the same scan and the global particle count. */
#define BPF_SHARD_NEED_BEAM_COUNTS 100
int bpf_shard_beam_counts_dev(bpf_engine* e, void** counts_dev, int* n_counts);
int bpf_shard_score_planar_finish(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                  double range_max, long long global_count);
/* the same for the 3-D path (PointCloudScanner::applyModelToSampleSet on the local shard) */
int bpf_shard_score_cloud(bpf_engine* e, const float* points_xyz, int n_points);
/* device address of the engine's scalar block, double[16]: [0] local weight total,
 * [1] w_slow, [2] w_fast, [7] local CDF sum (after bpf_shard_build_cdf) */
int bpf_shard_scalars_dev(bpf_engine* e, void** dev_ptr);
/* ParticleFilter::updateSensor's normalisation (particle_filter.cpp:237-266) with the global
 * total = totals_dev[0] + ... + totals_dev[world-1] (added in rank order) and the global count */
int bpf_shard_normalize_dev(bpf_engine* e, const void* totals_dev, int world, int global_sample_count);
/* local running sum c[0..n] of the shard's weights; its last element is copied to scalars[7];
 * flags_dev (nullable): an int the call zeroes, the CDF-miss flag of the draw windows that follow */
int bpf_shard_build_cdf(bpf_engine* e, void* flags_dev);
/* Candidate draws m in [m0, m1) of the multinomial resampler (particle_filter.cpp:381-414) from
 * the drand48 state `rng_state48`.  The shard owns the draws whose r lies in
 * [offset, offset + sums_dev[rank]) with offset = sums_dev[0] + ... + sums_dev[rank-1].
 * sums_are_totals = 1: sums_dev holds the gathered WEIGHT TOTALS of the last sensor update instead
 * (no second exchange): shard q's slice is then total_q / sum(totals), formed identically on every
 * rank; inside it the shard's own running sum is used and its last particle absorbs the rounding.
 * window_dev is int64[6][stride]: rows 0-2 the bit patterns of the selected pose (x, y, theta),
 * rows 3-5 its histogram key; column m - m0.  Owned draws are written, all others are zeroed, so
 * an integer sum over the ranks assembles the window exactly.  flags_dev[0] is set on a CDF miss. */
int bpf_shard_draw_window_dev(bpf_engine* e, uint64_t rng_state48, int m0, int m1, const void* sums_dev,
                              int sums_are_totals, int rank, int world, void* window_dev, int stride, void* flags_dev);
/* Tail of the sharded resample for a small set (global_count <= 8192), one launch: adopt poses
 * [lo, hi) of the assembled arrays with weight 1/global_count, flip the sets, and evaluate
 * updateConverged over all global_count poses. */
int bpf_shard_tail_small_dev(bpf_engine* e, const void* x_all_dev, const void* y_all_dev, const void* theta_all_dev,
                             int global_count, int lo, int hi, int leaf_count, int bin_count);
/* Become the resampled shard: copy `count` poses from device arrays, weight 1/global_count each
 * (particle_filter.cpp:409,458-462), flip the ping-pong sets. */
int bpf_shard_adopt_dev(bpf_engine* e, const void* x_dev, const void* y_dev, const void* theta_dev, int count,
                        int global_count, int leaf_count, int bin_count);
/* updateConverged (particle_filter.cpp:170-220) over the WHOLE resampled set (every rank holds it
 * after the window exchange); fetched lazily by bpf_pf_get_state. */
int bpf_shard_converged_dev(bpf_engine* e, const void* x_all_dev, const void* y_all_dev, int global_count);

/* ------------------------------------------------------------------ cluster statistics of a sharded set
 * computeClusterStatsForSet (particle_filter.cpp:505-636), PFKDTree::cluster (pf_kdtree.cpp:58-90,169-194) and
 * Node2D::getMaxWeightPose (node_2d.cpp:588-617) for the GLOBAL set S = the ranks' slices in rank order, without
 * moving the particles.  After the last stage bpf_pf_compute_cluster_stats, bpf_pf_get_cluster and
 * bpf_pf_get_max_weight_pose of this engine return, bit for bit, what ONE engine holding S returns -- same bins, same
 * components, same labels (a component's label is the rank of its earliest bin by GLOBAL sample index), the same ten
 * 32.96 fixed-point sums per cluster as exact integers, the same finishing arithmetic -- until this engine's slice
 * next changes.  Every stage that changes the slice's poses or weights (bpf_shard_update_action, the scoring stages,
 * bpf_shard_normalize_dev, bpf_shard_adopt_dev, bpf_shard_tail_small_dev, the one-call mailbox forms) drops the
 * installed result; the plain getters then evaluate THIS ENGINE'S SLICE ONLY (clusters cut at the shard boundary,
 * local labels, weights that sum to about 1 / world): that is not the global figure, run the stages again for it.
 * The stage functions are asynchronous on the engine's stream except where they return a count; no kernel waits for
 * another rank, the exchanges are the caller's, between the calls (a host without a transport of its own calls
 * bpf_shard_compute_cluster_stats / bpf_shard_get_max_weight_pose instead: the same stages over the engine's exchange).  Calls out of order, or after the slice changed,
 * return BPF_ERR_NOT_CONFIGURED.  Two forms, chosen by the GLOBAL count so that every rank chooses alike:
 *
 * Gathered form (global_count <= 4096, the tracking regime).  Crosses between ranks: one all-gather of the slices'
 * x / y / theta / weight (<= 128 KB), the caller's.  Redundant: every rank runs the single-block evaluation
 * (k_stats_block) on the whole set.  w_all NULL = every weight 1 / global_count (the set straight after a resample).
 * *handled_out: BPF_SHARD_STATS_INSTALLED; BPF_SHARD_STATS_DECLINED when the set holds more than 1024 bins or 64
 * clusters (use the distributed form); BPF_SHARD_STATS_HOST_ROUTE for a key outside the packing range, a non-finite
 * term, or BPF_OPT_STATS_HOST = 1 (use bpf_shard_stats_host).  All ranks see the same set, so they decide alike. */
/* the slice itself for that all-gather: device addresses of the current set's x / y / theta / weight arrays
 * (*count_out doubles each), valid until the next call that changes the set; work queued on the engine's stream has
 * to be ordered before a reader on another stream */
int bpf_shard_samples_dev(bpf_engine* e, void** x_dev, void** y_dev, void** theta_dev, void** w_dev, int* count_out);
#define BPF_SHARD_STATS_INSTALLED 1
#define BPF_SHARD_STATS_DECLINED 0
#define BPF_SHARD_STATS_HOST_ROUTE (-1)
int bpf_shard_stats_gathered_dev(bpf_engine* e, const void* x_all, const void* y_all, const void* theta_all,
                                 const void* w_all, int global_count, int* handled_out);
/* Distributed form, stage 1 (pf_kdtree.cpp:49-56, the bins of the slice): *bins_dev = int64[2][*n_bins_out] in engine
 * memory, row 0 the distinct packed bin keys of the slice, row 1 the GLOBAL index (global_first + local index) of each
 * key's first sample, in increasing first-index order.  *host_route_out = 1: a key outside the packing range, a
 * non-finite term, or BPF_OPT_STATS_HOST = 1 on this rank.  Crosses between ranks afterwards (exchange 1): the
 * counts with the host-route flags, then the lists padded to the largest count; if ANY rank raised the flag every
 * rank takes bpf_shard_stats_host instead.  Waits for the stream (the count comes back). */
int bpf_shard_stats_local_bins_dev(bpf_engine* e, long long global_first, void** bins_dev, int* n_bins_out,
                                   int* host_route_out);
/* Stage 2 (pf_kdtree.cpp:58-90,169-194), redundant on every rank: all_bins_dev = int64[world][2][pad], rank r's list
 * in its first counts[r] columns (world <= 16, counts in host memory).  One global bin table (a key held by several
 * ranks keeps its smallest first index), union-find over the 26 neighbours of each bin, labels by an exclusive scan
 * of "this bin is a root" over the bins in first-index order.  Waits for the stream. */
int bpf_shard_stats_label_dev(bpf_engine* e, const void* all_bins_dev, const int* counts, int world, int pad,
                              int* cluster_count_out);
/* Stage 3 (particle_filter.cpp:569-605 over the slice): every sample adds its ten terms to the accumulators of its
 * bin's cluster.  *sums_dev = int64[10 * cluster_count][4] in engine memory: each 128-bit sum as four 32-bit limbs,
 * least significant first, the top one signed, so that a lane-wise int64 sum over <= 16 ranks is exact.  Crosses
 * between ranks afterwards (exchange 2): an integer all-reduce(sum) of these *n_words_out words. */
int bpf_shard_stats_local_sums_dev(bpf_engine* e, void** sums_dev, size_t* n_words_out);
/* Stage 4 (particle_filter.cpp:541-567,607-635, node_2d.cpp:608-612), redundant on every rank: carries propagated,
 * the single engine's finishing kernels on the reduced sums, the result installed as this engine's statistics.
 * reduced_sums_dev may be the buffer stage 3 returned, reduced in place.  Waits for the stream.
 * The sums are 32.96 fixed point and end at |sum| < 2^31 (normalised weights: a cluster beyond ~46 km from the frame's
 * origin on one axis does not fit).  A rank whose own sums leave that range marks what it exports, and a total that
 * leaves it shows in the reduced words, so every rank finds out here, alike: nothing is installed then, the call
 * returns BPF_OK, bpf_shard_stats_finish_installed reports 0 and every rank takes bpf_shard_stats_host instead. */
int bpf_shard_stats_finish_dev(bpf_engine* e, const void* reduced_sums_dev);
int bpf_shard_stats_finish_installed(bpf_engine* e, int* installed_out);
/* The host route, redundant on every rank: particle_filter.cpp:505-636 in index order over the gathered set,
 * all_samples = global_count x (x, y, theta, w) in host memory; bit for bit the BPF_OPT_STATS_HOST = 1 evaluation of
 * one engine holding the set.  Crosses between ranks: the all-gather of the slices (32 B per particle), the caller's. */
int bpf_shard_stats_host(bpf_engine* e, const double* all_samples, int global_count);
/* ------------------------------------------------------------------ a sharded set initialised on its ranks
 * ParticleFilter::initWithGaussian (particle_filter.cpp:105-132) and ParticleFilter::initWithPoseFn (:135-163, the
 * global_localization service, node.cpp:870-882) for one shard: this engine writes samples
 * [global_first, global_first + local_count) of the set that ONE engine with max_samples = global_count and the same
 * rng state produces with bpf_pf_init_with_gaussian / bpf_pf_init_with_random_poses -- the same bits, weight
 * 1 / global_count -- and advances its rng by what the WHOLE set consumes, so every rank ends on the same state.
 * w_slow / w_fast are zeroed, the converged flag cleared, the slice becomes the current set (local_count 0: an empty
 * shard).  The set's histogram tree is NOT built: leaf_count / bin_count read -1 until bpf_shard_tree_merge_dev,
 * bpf_shard_tree_from_keys or a resample installs those of the GLOBAL set.  global_count must be the engine's
 * max_samples (BPF_ERR_INVALID_ARGUMENT).  The uniform pose check applies in its AS_REFERENCE form, with the capacity
 * refusals of the single call on the GLOBAL stream use; with BPF_POSE_CHECK_SENSOR_MODEL the random-pose form returns
 * BPF_ERR_UNSUPPORTED and touches nothing.  No exchange: every rank walks the same stream. */
int bpf_shard_init_with_gaussian(bpf_engine* e, const double mean[3], const double rotation[9], const double sigma[3],
                                 long long global_first, int local_count, long long global_count);
int bpf_shard_init_with_random_poses(bpf_engine* e, long long global_first, int local_count, long long global_count);
/* bpf_pf_init_with_mixture for one shard, in every respect as bpf_shard_init_with_gaussian: the counts are counts of
 * the GLOBAL set and sum to global_count, and a shard boundary may fall anywhere inside a component. */
int bpf_shard_init_with_mixture(bpf_engine* e, const bpf_mixture_component* comps, int n_components,
                                long long global_first, int local_count, long long global_count);
/* The histogram tree of the GLOBAL set (the PFKDTree initWith* builds, particle_filter.cpp:126-131,157-162, whose
 * leaf count the systematic resampler reads first, :285) without moving a particle: the shape of the tree depends
 * only on the order in which DISTINCT keys first appear (pf_kdtree.cpp:97-150), so the ranks exchange their bins.
 * local_bins: *bins_dev = int64[2][*n_bins_out] in engine memory, as bpf_shard_stats_local_bins_dev lists them (packed
 * keys, GLOBAL first indices, first-index order); *out_of_range_out = 1: a key of the slice does not fit the packing.
 * The statistics stages are not involved.  Crosses between ranks afterwards: the counts with the flags, then the
 * lists padded to the largest count (16 B per occupied bin).
 * merge (redundant on every rank; the slices must be contiguous in rank order): all_bins_dev = int64[world][2][pad],
 * rank r's list in its first counts[r] columns.  One table in which a key keeps its smallest first index, the
 * entries that are their key's first occurrence compacted in rank-then-list order, then the tree of those keys: the
 * device tree from 8 192 distinct keys on, the host tree below that or when the device tree declines; with
 * BPF_KLD_COUNT_BINS no tree, the leaf count is the bin count.  Installs leaf_count / bin_count where
 * bpf_shard_adopt_dev does.  Statistics stages in progress on this engine start over.  Waits for the stream.
 * If ANY rank raised out_of_range every rank takes the keys route instead: local_keys (*keys_dev = int32[*n_keys_out][3]
 * of the slice, in engine memory), an all-gather of those, and from_keys on the host copy of all of them in index
 * order -- correct and slow.  last_route: how the counts in force were found (0: none since the last init). */
enum
{
  BPF_SHARD_TREE_ROUTE_DEVICE = 1,    /* merged bins, device tree */
  BPF_SHARD_TREE_ROUTE_HOST = 2,      /* merged bins, host tree of the distinct keys */
  BPF_SHARD_TREE_ROUTE_BIN_COUNT = 3, /* merged bins, BPF_KLD_COUNT_BINS: no tree */
  BPF_SHARD_TREE_ROUTE_KEYS = 4       /* every raw key through the host tree */
};
int bpf_shard_tree_local_bins_dev(bpf_engine* e, long long global_first, void** bins_dev, int* n_bins_out,
                                  int* out_of_range_out);
int bpf_shard_tree_merge_dev(bpf_engine* e, const void* all_bins_dev, const int* counts, int world, int pad,
                             int* leaf_count_out, int* bin_count_out);
int bpf_shard_tree_local_keys_dev(bpf_engine* e, void** keys_dev, int* n_keys_out);
int bpf_shard_tree_from_keys(bpf_engine* e, const int* all_keys, int global_count, int* leaf_count_out,
                             int* bin_count_out);
int bpf_shard_tree_last_route(bpf_engine* e, int* route_out);
/* Advance a drand48 state by n draws (host arithmetic; the LCG jump the kernels use). */
uint64_t bpf_drand48_skip(uint64_t state48, uint64_t n);
/* Host-side exact KLD stop rule: replay ordered histogram keys through the fork's kd-tree
 * (pf_kdtree.cpp:97-150) and apply resampleLimit after each (particle_filter.cpp:416).
 * State persists in the engine between calls so windows can be fed one after another.
 * keys: int64 triples when keys_are_int64 != 0 (the window rows), else int32 triples, laid out
 * as three rows of `stride` (row-major [3][stride]). */
int bpf_kld_reset(bpf_engine* e);
int bpf_kld_feed(bpf_engine* e, const void* keys, int keys_are_int64, int stride, int n_keys, int first_draw_index,
                 int* stop_count_out);
/* the same with the keys still on the device: rows 3..5 of an assembled draw window (int64 [6][stride], see
 * bpf_shard_draw_window_dev).  A copy kernel on the engine's stream leaves them in pinned host memory behind a
 * generation word the host spins on (no D2H copy call, no stream synchronisation), then the replay runs. */
int bpf_kld_feed_dev(bpf_engine* e, const void* window_dev, int stride, int n_keys, int first_draw_index,
                     int* stop_count_out);
/* Brackets of a sharded resample.  begin: w_diff = max(0, 1 - w_fast / w_slow) from the engine's averages (the
 * same on every shard); for the multinomial resampler with w_diff > 0 it resolves where every candidate draw finds
 * its stream elements (kernels_recovery.hpp) -- bpf_shard_draw_window_dev then follows that chain and shard 0
 * writes the random free-space poses; *systematic_count_out = resampleLimit(leaf_count), grown by (1 + w_diff)
 * (particle_filter.cpp:295-306), the `count` to pass to bpf_shard_systematic_window_dev, whose first
 * int(w_diff * count) samples are random poses.  end: the drand48 state after `sample_count` samples, and the
 * reset of the averages when w_diff > 0 (:453-455).  Needs bpf_pf_set_random_pose_generator when w_diff > 0.
 * The uniform pose check of bpf_pf_set_uniform_pose_check applies in its AS_REFERENCE form; with
 * BPF_POSE_CHECK_SENSOR_MODEL begin returns BPF_ERR_UNSUPPORTED. */
int bpf_shard_begin_resample(bpf_engine* e, uint64_t rng_state48, int leaf_count, double* w_diff_out,
                             int* systematic_count_out);
int bpf_shard_end_resample(bpf_engine* e, int sample_count, uint64_t* rng_state48_out);
/* Systematic resampling over shards (particle_filter.cpp:269-354): the targets
 * start + m / count are formed on the host exactly as the reference's serial chain, every shard resolves the
 * targets that fall into its slice of the global CDF and writes pose bits + key into its window columns
 * (zeros elsewhere), as bpf_shard_draw_window_dev does for the multinomial draws.  count = what
 * bpf_shard_begin_resample returned; rng_state48 = state BEFORE the one drand48. */
int bpf_pf_resample_limit(bpf_engine* e, int leaf_count, int* count_out);
int bpf_shard_systematic_window_dev(bpf_engine* e, uint64_t rng_state48, int count, const void* sums_dev,
                                    int sums_are_totals, int rank, int world, void* window_dev, int stride,
                                    void* flags_dev);
/* Systematic resampling of a sharded set IN PLACE: every rank resamples its own slice into its own slice, and no draw
 * window crosses.  Opt-in (bpf_shard_set_resample_form); the default, BPF_SHARD_RESAMPLE_WINDOW, is the form above.
 * The multinomial resampler ignores the setting; it has an in-place form and a setting of its own
 * (bpf_shard_set_multinomial_form, below).
 *
 * Parity: a rotation of the reference's set.  Let S be the set ONE engine produces by resampleSystematic
 * (particle_filter.cpp:269-354) from the concatenation of the slices: n_random random poses first, then the teeth
 * i = 0 .. n - 1, whose targets the reference's serial chain forms (target += delta; if (target > 1.0) target -= 1.0)
 * exactly as bpf_shard_systematic_window_dev forms them.  With i_wrap the first tooth formed after the subtraction
 * (n when there is none), the in-place set is S[:n_random] + teeth[i_wrap:] + teeth[:i_wrap] -- the random poses, then
 * the teeth by ascending target -- as the concatenation of the new slices in rank order; every weight is 1 / M.
 *   ownership   shard q holds the teeth whose target lies in its slice [T_q, T_q+1) of the global CDF: the quotients
 *               and the ownership test of bpf_shard_draw_window_dev / bpf_shard_systematic_window_dev, so every tooth's
 *               source particle is the one the single engine picks (the shard's last particle absorbs the slice's
 *               rounding, the last shard whatever lies beyond the CDF, with the same miss flag).  Shard 0 also holds
 *               the random poses, at its head.  The slices come out uneven; a shard may end up empty.
 *   counts      every rank derives all W local counts from the totals and the targets: no exchange.
 *   drand48     bpf_shard_begin_resample / bpf_shard_end_resample as for the window form.
 *   tree        the leaf and bin counts of the new GLOBAL set by the bin-list route: bpf_shard_tree_local_bins_dev with
 *               the rank's new global_first, an all-gather of the lists, bpf_shard_tree_merge_dev (the keys route and
 *               BPF_KLD_COUNT_BINS included).
 *   converged   updateConverged over the global set: each rank forms exact 32.96 fixed-point sums of its x and y
 *               (order-independent), an integer all-reduce(sum) of the limb words, the mean from the reduced integers
 *               -- the same bits on every rank --, each rank's count within dist_threshold, a second integer all-reduce,
 *               then the single engine's float percentage test.  A non-finite or out-of-range term on any rank travels
 *               as a flag word in the first reduce and gives a count of 0, as the reference's comparisons against a NaN
 *               mean do.  (The single engine rounds its mean from a double sum; a particle within rounding of the
 *               threshold may be counted differently.)
 *   cap         max_share is a condition, not a measurement: when the largest local count would exceed
 *               max_share * ceil(M / W), every rank -- deciding alike from the redundant counts -- takes the window form
 *               for this resample, which re-splits evenly.  Default 2.0; max_share >= 1.  BPF_SHARD_REBALANCE_AUTO
 *               (below) lifts the cap and evens the slices out behind the resample instead.
 * What crosses between the ranks: the W totals (there already), 16 B per occupied bin, and ten integer words; the window
 * form sends 48 B per new sample to every rank.  That is a byte and operation count, not a measurement: nothing here
 * has run between two GPUs.
 *
 * Stage functions for a host with its own transport, after bpf_shard_build_cdf and bpf_shard_begin_resample:
 *   select      counts_out[world]: every rank's new local count; *global_first_out: this rank's first global index;
 *               *form_used_out: BPF_SHARD_RESAMPLE_IN_PLACE -- the new slice is current, its tree counts read -1 until
 *               the bin-list stages install them -- or BPF_SHARD_RESAMPLE_WINDOW: the cap applies, nothing was changed
 *               (the counts are the ones that were refused), go on with bpf_shard_systematic_window_dev.  Arguments as
 *               for bpf_shard_systematic_window_dev; sums_dev is read by the host (one small copy).
 *   xy_sums     *words_dev: n_words int64 words in engine memory (8 limbs and the flag) to all-reduce(sum) in place
 *   converged   reduced_words_dev: those words after the reduce; *count_dev: one int64 word to all-reduce(sum)
 *   finish      installs the reduced count; bpf_pf_get_state then reports converged.  Then bpf_shard_end_resample.
 * bpf_shard_update_resample takes the in-place form when it is set, over the mailbox, RCCL and the local exchange (four
 * small exchanges per resample whatever M is; *windows_out = 0); every exchange is finished before the new slice becomes
 * current, so BPF_ERR_EXCHANGE leaves the set as it was.
 * bpf_shard_slice: where this engine's slice sits in the global set as the last sharded init, bpf_shard_tail_small_dev,
 * in-place select or one-call resample left it, and the form the last resample used; BPF_ERR_NOT_CONFIGURED when the
 * set came from somewhere else (bpf_pf_set_samples, bpf_shard_adopt_dev, bpf_pf_restore, an unsharded
 * bpf_pf_update_resample). */
enum
{
  BPF_SHARD_RESAMPLE_WINDOW = 0,
  BPF_SHARD_RESAMPLE_IN_PLACE = 1
};
int bpf_shard_set_resample_form(bpf_engine* e, int form, double max_share);
int bpf_shard_get_resample_form(const bpf_engine* e, int* form_out, double* max_share_out);
int bpf_shard_slice(bpf_engine* e, long long* global_first_out, int* local_count_out, int* form_used_out);
int bpf_shard_inplace_select_dev(bpf_engine* e, uint64_t rng_state48, int count, const void* sums_dev,
                                 int sums_are_totals, int rank, int world, void* flags_dev, int* counts_out,
                                 long long* global_first_out, int* form_used_out);
int bpf_shard_inplace_xy_sums_dev(bpf_engine* e, void** words_dev, size_t* n_words_out);
int bpf_shard_inplace_converged_dev(bpf_engine* e, const void* reduced_words_dev, int global_count, void** count_dev);
int bpf_shard_inplace_converged_finish(bpf_engine* e, const void* reduced_count_dev, int global_count);
/* Multinomial resampling of a sharded set IN PLACE: every rank resamples its own slice into its own slice, and the KLD
 * stop index comes from the ranks' bin lists.  Opt-in through a setting of its own (bpf_shard_set_multinomial_form;
 * bpf_shard_set_resample_form means what it meant: with the multinomial resampler it changes nothing).  max_share and
 * the rebalance setting are the ones of bpf_shard_set_resample_form / bpf_shard_set_rebalance.
 *
 * Model.  Draws are numbered m = 0 .. max_samples - 1; draw m reads fixed elements of the drand48 stream (2 m + 1 and
 * 2 m + 2, or the recovery chain's when w_diff > 0), so every rank can evaluate every candidate draw.
 *   candidates  a CDF draw belongs to the rank whose ownership test (bpf_shard_draw_window_dev's) accepts its uniform, a
 *               random pose of w_diff > 0 to rank 0.  A rank keeps its owned draws in ascending draw index: pose bits
 *               and the draw index.  Every rank evaluates max_samples candidates, not max_samples / W: that redundant
 *               work is the price of having no window.
 *   bin lists   the distinct keys of the kept draws, each with the smallest draw index under that key: 16 B per
 *               occupied bin.  They cross once, with the (bin count, key-outside-the-packing flag) words.
 *   stop        merged by key with the minimum draw index: B distinct keys with first draw indices t_0 < ... < t_{B-1},
 *               t_B = max_samples.  The tree is a function of the distinct keys in first-occurrence order, so inserting
 *               them in that order gives L_j, the leaf count after the j-th (BPF_KLD_COUNT_BINS: L_j = j + 1).  With
 *               c_j = max(t_j + 1, resampleLimit(L_j) + 1), M is the smallest c_j <= t_{j+1}, and the leaf and bin
 *               counts of the new set are L_j and j + 1 there; if no j qualifies M = max_samples with L_{B-1} and B.
 *               (The first branch of c_j is the draw that adds key j itself: it decides where the leaf count falls
 *               with a new key.)  Every rank computes this from the same merged list; B >= 8192 takes the device tree,
 *               fewer keys -- or a list the device tree declines -- the host tree.
 *   truncate    rank q's new slice is its kept draws with index < M, in draw order; weights 1 / M.  The concatenation
 *               of the slices in rank order is the reference's S[0:M] sorted stably by (owner, draw index): the same
 *               multiset, a permutation.  What follows (the motion update's per-index Gaussians, ...) follows the
 *               permuted order.
 *   counts      every rank derives all W local counts by counting the owners of draws 0 .. M - 1: no exchange.
 *   cap         as for the systematic form: when the largest count exceeds max_share * ceil(M / W) nothing has been
 *               changed and the window form takes this resample; BPF_SHARD_REBALANCE_AUTO lifts the cap and evens the
 *               slices out behind the committed resample.
 *   converged, drand48, w_slow / w_fast
 *               as for the systematic form: the limb-word and count reduces, bpf_shard_end_resample(M).
 *   miss        a candidate beyond the stop is a draw the reference never made: the miss flag is raised only when the
 *               smallest draw index whose search failed lies below M.
 *   keys route  a key outside the 64-bit packing would need the draw indices beside the raw keys; the one-call form
 *               takes the window form for that resample instead, and a staged host does the same when
 *               bpf_shard_inplace_mn_bins_dev reports *out_of_range_out = 1 on any rank.
 * Four exchanges per resample whatever M is -- the count and flag words, the bin lists, the limb words, the converged
 * count -- and a fifth when the AUTO rebalance runs; the window form sends 48 B per new sample to every rank and replays
 * all M keys on every rank.  That is a byte and operation count, not a measurement: nothing here has run between two
 * GPUs.
 *
 * Stage functions for a host with its own transport, after bpf_shard_build_cdf and bpf_shard_begin_resample; a stage
 * called out of order answers BPF_ERR_NOT_CONFIGURED:
 *   select   writes the kept candidates into the set that is not current; *n_kept_out of them.  Refuses the systematic
 *            resampler and a resample that was not begun with this rng_state48 (BPF_ERR_INVALID_ARGUMENT).
 *   bins     *bins_dev = int64[2][*n_bins_out] in engine memory: packed keys, first draw indices
 *   stop     all_bins_dev = the gathered lists int64[world][2][pad], counts[world] their lengths.  Merges, finds the
 *            stop, counts the owners (counts_out[world]) and applies the cap: *form_used_out =
 *            BPF_SHARD_RESAMPLE_WINDOW means nothing was changed (go on with bpf_shard_draw_window_dev), else the new
 *            slice is current with the global set's tree counts.
 *   then bpf_shard_inplace_xy_sums_dev / _converged_dev / _converged_finish and bpf_shard_end_resample(M).
 * bpf_shard_update_resample takes this form for the multinomial resampler when the setting is
 * BPF_SHARD_RESAMPLE_IN_PLACE, over the mailbox, RCCL and the local exchange (*windows_out = 0; the mailbox windows may
 * be smaller than max_samples); every exchange is finished before the new slice becomes current, so BPF_ERR_EXCHANGE
 * leaves the set as it was.  bpf_shard_slice reports form_used = BPF_SHARD_RESAMPLE_IN_PLACE. */
int bpf_shard_set_multinomial_form(bpf_engine* e, int form);
int bpf_shard_get_multinomial_form(const bpf_engine* e, int* form_out);
int bpf_shard_inplace_mn_select_dev(bpf_engine* e, uint64_t rng_state48, const void* sums_dev, int sums_are_totals,
                                    int rank, int world, void* flags_dev, int* n_kept_out);
int bpf_shard_inplace_mn_bins_dev(bpf_engine* e, void** bins_dev, int* n_bins_out, int* out_of_range_out);
int bpf_shard_inplace_mn_stop_dev(bpf_engine* e, const void* all_bins_dev, const int* counts, int world, int pad,
                                  int* sample_count_out, int* leaf_count_out, int* bin_count_out, int* counts_out,
                                  long long* global_first_out, int* form_used_out);
/* Rebalancing the slices of a sharded set: the other half of the in-place form.  The slices go back to the even split
 * in GLOBAL order -- the concatenation of the slices in rank order is the same before and after, bit for bit, x, y,
 * theta and weight -- and only the samples that sit on the wrong rank move.  Opt-in; nothing calls it unless asked.
 *
 * The plan is a pure function of the W local counts (contiguous shards), so every rank derives the same one with no
 * exchange.  With counts[0 .. W), G = sum(counts), W <= 16:
 *   old prefix  P[r] = counts[0] + ... + counts[r - 1]; rank r holds the global indices [P[r], P[r + 1])
 *   new prefix  Q[r] = (G r) / W in integer arithmetic -- the even split of every re-split here,
 *               (M (r + 1)) / W - (M r) / W samples on rank r; rank r's new slice is [Q[r], Q[r + 1])
 *   kept        rank r keeps [max(P[r], Q[r]), min(P[r + 1], Q[r + 1])); when that is empty, the empty range at P[r]
 *   outgoing    the rest of its old slice in ascending global index, a head span and then a tail span:
 *               out[r] = counts[r] - kept[r] samples; T = sum(out).  T = 0: the split is even already
 *   sources     global index g of rank r's new slice is owned by the rank q with P[q] <= g < P[q + 1]; q = r: the
 *               local sample g - P[r]; else entry g - P[q] of q's outgoing list when g lies below q's kept range and
 *               entry g - P[q] - kept[q] when it lies above
 * What crosses: one ragged all-gather of the outgoing rows, int64[4][out[r]] per rank (the bit patterns of x, y, theta,
 * w).  The gather is a broadcast, so 32 T bytes enter EVERY rank.  A point-to-point form, in which a moved particle
 * enters one rank only, is not built.  That is a byte count, not a measurement: nothing here has run between two GPUs.
 *
 * State (one transition): the other buffer becomes current with the new sample count, bpf_shard_slice answers with
 * Q[rank], the new count and G; the CDF and partials, the cached statistics and the W totals of the last sensor update
 * (they belong to the old split) are dropped.  What describes the GLOBAL set or the filter stays: leaf and bin counts
 * and their route (pending counts stay pending), converged, w_slow / w_fast, the drand48 state, the form the last
 * resample used.
 *
 * bpf_shard_rebalance: one collective call over the engine's own exchange (mailbox, RCCL, local): one gather of one
 * word per rank for the local counts; if T > 0 the pack, a second gather of the rows into a compact int64[4][T], then
 * the assemble and the transition.  *moved_out = T, the same on every rank.  bpf_shard_exchange_count rises by 2 when
 * something moves and by 1 when nothing does.  T = 0: the set, its epoch and its caches are untouched, except that
 * where the slice sits is recorded from the gathered counts (bpf_shard_slice then answers).
 *   atomicity   every exchange is finished before the transition: on BPF_ERR_EXCHANGE or BPF_ERR_CAPACITY (mailbox:
 *               the rows need 4 T <= 6 max_window words) the old slice stays current with all its state.
 *
 * Stage functions for a host with its own transport; no call waits for another rank:
 *   plan        counts[world]: every rank's local count, the same array on every rank.  out_counts[world]: out[];
 *               *new_first_out = Q[rank], *new_count_out = Q[rank + 1] - Q[rank].  Records the plan in the engine and
 *               changes nothing else.  BPF_ERR_INVALID_ARGUMENT: world outside 1 .. 16, rank outside [0, world), a
 *               negative count, counts[rank] != this engine's sample count, G > max_samples.
 *   export      packs this rank's outgoing list: *rows_dev = int64[4][out[rank]] with row stride out[rank] (engine
 *               memory, valid until the next rebalance call; a pointer even when *n_out = 0)
 *   import      rows_dev: the gathered rows, rank q's row k (x, y, theta, w) at rank_off[q] + k * row_stride, in device
 *               memory that stays as it is until the engine's stream has passed this call; assembles the new slice and
 *               makes the transition.  out[] all zero: a no-op for the set (rows_dev may be null); the slice's place
 *               is recorded as the one-call form does.
 *   export and import belong to the plan of the CURRENT set: after anything that changed the set since
 *   bpf_shard_rebalance_plan (a motion or sensor update, a resample, a rebalance) they return BPF_ERR_NOT_CONFIGURED.
 *
 * bpf_shard_set_rebalance, BPF_SHARD_REBALANCE_AUTO: applies to bpf_shard_update_resample (and the staged select) on
 * the systematic in-place path only, BPF_SHARD_RESAMPLE_IN_PLACE set.  The max_share cap then no longer sends a
 * resample to the window form: the select always runs in place (a new slice never exceeds count <= max_samples).  After
 * the resample is complete and committed, if the largest new count exceeds trigger_share * ceil(M / W), the rebalance
 * above runs -- every rank decides alike from the resample's own counts, so no count crosses: five exchanges per
 * resample instead of four.  A rebalance whose exchange fails returns the error; the resampled, uneven set stays current
 * and valid.  The staged select only lifts the cap; its host runs the stage functions above.  Default
 * BPF_SHARD_REBALANCE_OFF: the behaviour without this section exactly, cap included.  trigger_share >= 1, default 1.5:
 * a policy condition, not a measurement.  trigger_share < 1 or a NaN: BPF_ERR_INVALID_ARGUMENT.  The multinomial
 * resampler and the window form re-split evenly themselves and are untouched.
 * bpf_shard_rebalance_last: T of the last rebalance this engine completed (0 when the last AUTO resample found nothing
 * to do, and 0 after a rebalance that failed: nothing has moved then; *moved_out of bpf_shard_rebalance likewise).
 * bpf_shard_resample_committed: with AUTO, bpf_shard_update_resample can return an error AFTER its resample became
 * current (the rebalance behind it failed).  *committed_out = 1 when the last bpf_shard_update_resample /
 * bpf_shard_mailbox_update_resample of this engine made its new set current, whatever it returned; the count, leaf and
 * bin outputs were written then.  A caller that sees an error with committed = 1 must NOT run the resample again: it
 * refreshes its record of the split (bpf_shard_slice) and, if it wants even slices, calls a rebalance.  Without AUTO an
 * error always means committed = 0.
 *
 * Between a sensor update and a resample a rebalance keeps the normalised weights (they are copied) but drops the W
 * totals: the one-call bpf_shard_update_resample then answers BPF_ERR_NOT_CONFIGURED, as for any update without
 * totals, and leaves the set alone; a staged host gathers the local CDF sums instead (sums_are_totals = 0).  AUTO never
 * rebalances there. */
enum
{
  BPF_SHARD_REBALANCE_OFF = 0,
  BPF_SHARD_REBALANCE_AUTO = 1
};
int bpf_shard_set_rebalance(bpf_engine* e, int mode, double trigger_share);
int bpf_shard_get_rebalance(const bpf_engine* e, int* mode_out, double* trigger_share_out);
int bpf_shard_rebalance_last(const bpf_engine* e, long long* moved_out);
int bpf_shard_resample_committed(const bpf_engine* e, int* committed_out);
int bpf_shard_rebalance(bpf_engine* e, long long* moved_out);
int bpf_shard_rebalance_plan(bpf_engine* e, const long long* counts, int rank, int world, long long* out_counts,
                             long long* new_first_out, int* new_count_out);
int bpf_shard_rebalance_export_dev(bpf_engine* e, void** rows_dev, long long* n_out);
int bpf_shard_rebalance_import_dev(bpf_engine* e, const void* rows_dev, const long long* rank_off,
                                   long long row_stride);
/* Mailbox exchange: the two small exchanges of the sharded path (W weight totals; one draw window whose every
 * column has exactly one writer) without a collective library.  Every engine of the node owns one uncached device
 * allocation, exported by IPC handle and mapped by the W - 1 others; a producer kernel stores its values into the
 * same slot of every peer's mailbox over xGMI and then a generation word (system-scope release), a consumer kernel
 * waits on the words in its own mailbox (bounded: 5 s, then BPF_ERR_EXCHANGE at the next host check).  The post
 * rides on the kernel that produces the value and the wait on the kernel that consumes it: no extra launch and no
 * host round trip.  Stands where torch.distributed / RCCL all-gather + all-reduce would (badger_amcl_amd/sharded.py
 * falls back to those when a mailbox cannot be set up); there is no counterpart in the reference.
 *   create   allocates for windows of up to max_window draws and returns the 64-byte IPC handle;
 *   connect  takes the world x 64 bytes of all ranks' handles in rank order (gather them with any host-side
 *            transport), maps the peers and runs one post-and-wait round with all of them -- every rank must call
 *            it at about the same time; BPF_ERR_EXCHANGE when a peer does not answer;
 *   totals   after a sharded scoring stage: device pointer to the W totals of this update, to be passed as
 *            totals_dev / sums_dev.  This rank's total is posted to the peers by the scoring stage or, for the field
 *            models, by the bpf_shard_normalize_dev launch that must follow (it folds the scoring kernel's partials,
 *            posts, and then waits in-kernel for all W totals);
 *   window   a fresh [6][stride] int64 window for the next exchange: bpf_shard_draw_window_dev /
 *            bpf_shard_systematic_window_dev given this pointer store every owned column into all peers' copies, and
 *            the first consumer (bpf_kld_feed_dev / bpf_kld_insert_dev / bpf_kld_stop_dev) waits for all shards.
 *            The window stays valid until the next-but-one call; copy out what has to live longer.
 * The one-call forms further down (bpf_shard_update_sensor_planar with beam skipping, bpf_shard_compute_cluster_stats,
 * bpf_shard_get_max_weight_pose) send their small payloads through the same window region, addressed by word offset:
 * ragged all-gathers (every rank's span in rank order) and an integer all-reduce as gather-then-sum in rank order.
 * They take window generations of their own, so a window handed out by bpf_shard_mailbox_window must have been
 * consumed before one of them is called. */
/* A wait is bounded (default 5 s; set before create / connect).  When a bound runs out the consumer kernel leaves its
 * data alone -- after a failed wait for the totals the weights stay scored but NOT normalised, the local total in
 * bpf_shard_scalars_dev [0]; a failed window wait touches nothing of the current set -- and the next host check returns
 * BPF_ERR_EXCHANGE.  bpf_shard_mailbox_error_stage says which exchange it was, so that a driver can finish the update
 * over its other transport (all-gather the local totals, bpf_shard_normalize_dev, resample with collectives) and set
 * the mailbox up again: badger_amcl_amd/sharded.py does exactly that. */
int bpf_shard_mailbox_set_timeout_ms(bpf_engine* e, int timeout_ms);
int bpf_shard_mailbox_error_stage(bpf_engine* e, int* totals_failed, int* window_failed);
#define BPF_MAILBOX_HANDLE_BYTES 64
int bpf_shard_mailbox_create(bpf_engine* e, int rank, int world, long long max_window, void* handle_out);
int bpf_shard_mailbox_connect(bpf_engine* e, const void* handles);
/* Mailbox mode, the sharded sensor update and resample as one call each: what badger_amcl_amd/sharded.py does with
 * the stage functions above, in the same order, with the exchanges inside the kernels -- so that a host pays one
 * call per update.  update_sensor: bpf_shard_score_planar + totals + bpf_shard_normalize_dev (returns
 * BPF_SHARD_NEED_BEAM_COUNTS unchanged when beam skipping needs the caller's all-reduce: finish with the stage
 * functions then).  update_resample: multinomial (windows sized from *window_hint_io, follow-up windows, whole-stream
 * device tree) or systematic; *global_count_io / *leaf_count_io: the global sample count and the leaf count of the
 * current set's tree in, those of the new set out; this rank adopts its even share [M r / W, M (r + 1) / W);
 * flags_dev as in bpf_shard_build_cdf / bpf_shard_draw_window_dev (int32[>= 1] on the device, [0] = CDF-miss flag). */
int bpf_shard_mailbox_update_sensor_planar(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                           double range_max, long long global_count);
int bpf_shard_mailbox_update_resample(bpf_engine* e, void* flags_dev, int* global_count_io, int* leaf_count_io,
                                      int* bin_count_out, int* windows_out, int* window_hint_io);
/* `rounds` full window exchanges with a checkable payload (every rank writes a pattern into its share of the columns
 * of every peer, every rank verifies all columns after the wait); all ranks must call it together, after connect.
 * BPF_ERR_EXCHANGE when a cell did not arrive as written or a wait ran out. */
int bpf_shard_mailbox_selftest(bpf_engine* e, int rounds);
int bpf_shard_mailbox_destroy(bpf_engine* e);
int bpf_shard_mailbox_totals(bpf_engine* e, void** totals_dev);
int bpf_shard_mailbox_window(bpf_engine* e, void** window_dev, int* stride);
/* Bring-up of a sharded filter from a plain C / C++ host (no Python, no MPI, no launcher): every rank of the node calls
 * bpf_shard_bootstrap with the same "host:port".  Rank 0 listens there, the others connect (TCP inside this library);
 * over those sockets the ranks gather the mailbox IPC handles, map each other's mailboxes, run the connect round and the
 * self-test and agree on the result.  When the mailbox cannot be used on every rank they all fall back to RCCL:
 * libbadger_pf_rccl.so (linked against librccl, loaded only then) joins a communicator whose unique id rank 0 hands out
 * over the same sockets, and the two exchanges become ncclAllGather (totals) and an integer ncclAllReduce (windows).
 * *mode_out: which one it is.  flags: BPF_BOOTSTRAP_FORCE_COLLECTIVE skips the mailbox, BPF_BOOTSTRAP_MAILBOX_ONLY
 * fails instead of falling back.  The sockets are closed before the call returns.  The engine must carry the GLOBAL
 * min / max sample counts (bpf_pf_create) and this rank's shard of the set. */
enum
{
  BPF_SHARD_EXCHANGE_MAILBOX = 1,
  BPF_SHARD_EXCHANGE_RCCL = 2,
  BPF_SHARD_EXCHANGE_LOCAL = 3
};
enum
{
  BPF_BOOTSTRAP_FORCE_COLLECTIVE = 1,
  BPF_BOOTSTRAP_MAILBOX_ONLY = 2
};
int bpf_shard_bootstrap(bpf_engine* e, int rank, int world, const char* host_port, long long max_window, int flags,
                        int* mode_out);
int bpf_shard_shutdown(bpf_engine* e);
/* All ranks of ONE sharded filter inside this process (a single-process node with several engines): engines[r] becomes
 * rank r of `world`.  One thread calls it, once; no sockets, no IPC handles, no RCCL.  1 <= world <= 16, the engines
 * distinct, each after bpf_pf_create with the same (GLOBAL) min / max sample counts, on one device or on devices with
 * peer access both ways (which the call enables); flags must be 0.  Anything else returns BPF_ERR_INVALID_ARGUMENT or
 * BPF_ERR_UNSUPPORTED (no peer access) and leaves every engine as it was.  A mailbox or RCCL set-up on the engines is
 * released first, as bpf_shard_bootstrap does; an earlier local world too.
 * Afterwards every collective one-call form (bpf_shard_update_*, bpf_shard_*_all, bpf_shard_compute_cluster_stats,
 * bpf_shard_get_*, bpf_shard_global_leaf_count) works unchanged, with this calling convention: all `world` ranks
 * enter the same call concurrently, ONE HOST THREAD PER ENGINE (an engine itself stays single-threaded).  The ranks
 * meet at a host barrier inside every exchange; the data moves by one launch per rank that reads the peers' buffers,
 * ordered by events between the engines' streams -- no kernel waits for another rank.  bpf_shard_exchange_count counts
 * as on the RCCL path.  A rank that does not arrive within bpf_shard_mailbox_set_timeout_ms (default 5 s) breaks the
 * world: the waiting ranks return BPF_ERR_EXCHANGE with their destinations untouched, and every later exchange fails at
 * once until the next bpf_shard_connect_local.  bpf_shard_shutdown and bpf_destroy detach an engine (the world is
 * broken for the ranks that stay); the last one out frees the world. */
int bpf_shard_connect_local(bpf_engine* const* engines, int world, int flags);
/* *mode_out: 0 (no exchange set up), BPF_SHARD_EXCHANGE_MAILBOX, _RCCL or _LOCAL */
int bpf_shard_exchange_mode(const bpf_engine* e, int* mode_out);
/* Self-test of the local transport (collective, like bpf_shard_mailbox_selftest): ragged int64 gathers with one rank
 * contributing nothing and spans off the 16-byte grid, f64 all-gathers, int64 and int32 all-reduces in place at every
 * offset within 16 bytes, each at 0, 1, 255, 256, 257 and 6 * 4096 + 3 words, every cell and the guard words around
 * the destinations compared on the host.  BPF_ERR_EXCHANGE on a difference (the world is then broken). */
int bpf_shard_local_selftest(bpf_engine* e, int rounds);
/* Measurement (tools/time_local_world.py): `reps` exchanges of one kind back to back over the engine's collective
 * provider (the local world, or RCCL after the bootstrap's fallback), the host's wall time per exchange between two
 * stream synchronisations.  kind 0: f64 all-gather of `words` words per rank (1 = the totals); kind 1: int64
 * all-reduce(sum) of `words` words (6 * 4096 = a draw window).  Collective: every rank, the same arguments. */
int bpf_shard_exchange_probe(bpf_engine* e, int kind, long long words, int reps, double* ms_per_exchange_out);
/* The sharded sensor update and resample as one call each, over whichever exchange bpf_shard_bootstrap (or
 * bpf_shard_mailbox_connect) set up; arguments as bpf_shard_mailbox_update_sensor_planar / _update_resample, with the
 * CDF-miss flag word owned by the engine (*cdf_miss_out, nullable, reads it back).
 * bpf_shard_update_sensor_planar is NOT an alias of the mailbox form: with the prob model's beam skipping active it
 * sums the per-beam counts over the engine's own exchange between the two passes (mailbox: gather-then-sum of
 * max_beams words through the window region; RCCL: an int32 all-reduce) and finishes the update, where
 * bpf_shard_mailbox_update_sensor_planar hands BPF_SHARD_NEED_BEAM_COUNTS back to a caller with a transport of its
 * own.  It never returns BPF_SHARD_NEED_BEAM_COUNTS. */
int bpf_shard_update_sensor_planar(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                   double range_max, long long global_count);
int bpf_shard_update_resample(bpf_engine* e, int* global_count_io, int* leaf_count_io, int* bin_count_out,
                              int* windows_out, int* window_hint_io, int* cdf_miss_out);
/* PointCloudScanner::updateSensor (point_cloud_scanner.cpp:92-102) over the shards, as bpf_pf_update_sensor_cloud has
 * it for one engine: bpf_shard_score_cloud, the exchange of the W totals, bpf_shard_normalize_dev.  Leaves what
 * bpf_shard_update_resample requires of "the totals of this update". */
int bpf_shard_update_sensor_cloud(bpf_engine* e, const float* points_xyz, int n_points, long long global_count);
/* The statistics of the GLOBAL set in one collective call (every rank, in the same order): the stage functions of
 * "cluster statistics of a sharded set" above, in the order badger_amcl_amd/sharded.py runs them, with the engine's
 * own exchanges between them -- the local sample counts, then by the GLOBAL count the gathered form (<= 4096: the
 * slices' x / y / theta / weight) or the distributed form (the bin counts with the host-route flags, the bin lists, the
 * limb words of the per-cluster sums as an exact integer all-reduce, in rounds when they exceed the window region);
 * the host route (the slices, 32 B per particle) when any rank raises the flag or the gathered form asks for it.
 * Afterwards bpf_pf_get_cluster and the plain getters of THIS engine return the global figures, the same bits on
 * every rank, until the slice next changes.  Lazy: a second query while no slice has changed makes no exchange
 * (bpf_shard_exchange_count stays).  *route_out (nullable): which form evaluated the figures in force.
 * BPF_ERR_NOT_CONFIGURED without an exchange; BPF_ERR_EXCHANGE after a mailbox wait that ran out -- the set and any
 * statistics installed before are untouched, and bpf_shard_mailbox_error_stage reports these waits as the window
 * kind. */
enum
{
  BPF_SHARD_STATS_ROUTE_GATHERED = 1,
  BPF_SHARD_STATS_ROUTE_DISTRIBUTED = 2,
  BPF_SHARD_STATS_ROUTE_HOST = 3
};
int bpf_shard_compute_cluster_stats(bpf_engine* e, int* cluster_count_out, double set_mean[3], double set_cov[5],
                                    int* route_out);
/* Node2D::getMaxWeightPose over the global set (the same evaluation, the same laziness) */
int bpf_shard_get_max_weight_pose(bpf_engine* e, double* max_weight, double pose[3]);
/* The sharded inits as one collective call each (every rank, same arguments, same rng state): this rank takes its
 * even share [G r / W, G (r + 1) / W) of G = max_samples (the split the resample re-split uses, rank / world of
 * bpf_shard_bootstrap or bpf_shard_mailbox_connect), runs the stage form above and then the global tree over the
 * engine's own exchange: one gather of the bin counts with the out-of-range flags, one of the ragged bin lists (2
 * words per bin through the window region), the merge; or, when any rank raised the flag, the slices and the keys
 * route.  Afterwards every rank holds its slice, the common rng state and the leaf / bin counts of the global set.
 * BPF_ERR_EXCHANGE after a failed exchange: rng, set and counts are as before the call. */
int bpf_shard_init_with_gaussian_all(bpf_engine* e, const double mean[3], const double rotation[9],
                                     const double sigma[3]);
int bpf_shard_init_with_random_poses_all(bpf_engine* e);
int bpf_shard_init_with_mixture_all(bpf_engine* e, const bpf_mixture_component* comps, int n_components);
/* Leaf and bin count of the GLOBAL set's tree for slices loaded by hand (bpf_pf_set_samples on every rank, call this
 * before the first motion update): the local sample counts, then the exchanges above.  While counts of the global
 * set are in force (after one of the inits above, this call or a sharded resample) it returns them without an
 * exchange. */
int bpf_shard_global_leaf_count(bpf_engine* e, int* leaf_count_out, int* bin_count_out);
/* Diagnostic: exchanges this engine has issued since bpf_shard_bootstrap (or bpf_shard_mailbox_connect) set the
 * exchange up -- totals, draw windows, gathers and reduce rounds together. */
int bpf_shard_exchange_count(bpf_engine* e, long long* out);

/* ------------------------------------------------------------------ the particle cloud, formed on the device
 * Node::publishParticleCloud (node.cpp:335-357) loops over set->sample_count samples after every scanner update
 * (node_2d.cpp:384-385, node_3d.cpp:363-364), q.setRPY(0, 0, theta) and one geometry_msgs::Pose each.  These calls
 * replace that loop: PoseArray entries {x, y, 0, qx, qy, qz, qw} = {x, y, 0, 0, 0, sin(theta / 2), cos(theta / 2)}, the
 * layout and the arithmetic of bpf_wire_samples_to_pose_array, written by one kernel and read back in one copy.  x and y
 * are the set's bits, the three zeros are +0.0, sin / cos are the device's (within a few units in the last place of
 * libm's).  The header (stamp, frame id) stays with the caller.
 *
 * For all four: stride < 1, first < 0, a root outside [-1, world) or a null output on a receiving rank return
 * BPF_ERR_INVALID_ARGUMENT; capacity (in poses) < count returns BPF_ERR_CAPACITY and leaves poses7_out alone; without a
 * filter (the sharded one-call form: or without an exchange) BPF_ERR_NOT_CONFIGURED; an empty selection is BPF_OK with
 * count 0.  Read-only for the filter: set, weights, statistics in force, tree counts, the CDF hand-over and the
 * drand48 state stay as they were, and no buffer of another stage is borrowed.  poses7_out inside a
 * bpf_host_buffer_register'ed range is written by the copy engine directly (keep one PoseArray alive and register
 * its storage once); pageable memory goes through the engine's pinned bounce buffer.  On return the copy is complete. */
/* Node::publishParticleCloud's poses from the RESIDENT set: pose k = sample first + k * stride, k = 0 .. count-1,
 * count = first < n ? (n - first + stride - 1) / stride : 0.  first = 0, stride = 1 is the reference's message.   */
int bpf_pf_get_pose_array(bpf_engine* e, int first, int stride, double* poses7_out, int capacity, int* count_out);
/* Stage forms for a host with its own transport (node.cpp:335-357 over a sharded set).  rows: the x / y / theta bits
 * of the samples of THIS slice (which starts at global index global_first) that the selection first, first + stride,
 * ... of the GLOBAL index space picks, as int64[3][n_rows] with row stride n_rows, in index order (engine memory,
 * valid until the next pose-array call).  The caller concatenates the ranks' rows in rank order ... */
int bpf_shard_pose_rows_dev(bpf_engine* e, long long global_first, long long first, int stride,
                            void** rows_dev, int* n_rows_out);          /* int64[3][n_rows] of this slice        */
/* ... and any engine forms the n poses from the gathered rows int64[3][n] with row stride row_stride (device memory) */
int bpf_pose_array_from_rows_dev(bpf_engine* e, const void* rows_dev, long long row_stride, int n,
                                 double* poses7_out, int capacity);     /* any engine; no filter needed          */
/* One call over the engine's own exchange (after bpf_shard_bootstrap); collective: every rank calls it with the
 * same root / first / stride.  root >= 0: that rank receives, the others may pass poses7_out = NULL;
 * root = -1: every rank receives.  count_out is set on every rank.  (node.cpp:335-357 on the publishing rank.)
 * Two exchanges: the local sample counts, from which every rank derives every rank's share of the selection, then
 * one ragged gather of the rows (3 words per selected pose); every rank takes part in both, only receivers form and
 * read back.  Legal wherever bpf_shard_get_max_weight_pose is; makes no exchange for an empty selection beyond the
 * counts.  BPF_ERR_EXCHANGE after a mailbox wait that ran out, BPF_ERR_CAPACITY when the rows exceed the mailbox's
 * window region: the output is untouched. */
int bpf_shard_get_pose_array(bpf_engine* e, int root, long long first, int stride, double* poses7_out,
                             int capacity, int* count_out);
/* insert every key of the window into the engine's histogram tree (no stop rule): the tree of a systematic
 * resample, or of an initial set (keys as bpf_kld_feed / bpf_kld_feed_dev take them) */
int bpf_kld_insert(bpf_engine* e, const void* keys, int keys_are_int64, int stride, int n_keys);
int bpf_kld_insert_dev(bpf_engine* e, const void* window_dev, int stride, int n_keys);
/* the stop rule for a WHOLE candidate stream (draws 0 .. n_keys-1, keys in rows 3..5 of the device window)
 * evaluated on the device (level-synchronous build of the same kd-tree).
 * *handled_out = 0 when a key does not fit the 64-bit packing or the tree is deeper than 256 levels: feed the
 * stream through bpf_kld_feed_dev instead.  *stop_count_out = -1: no stop up to n_keys. */
int bpf_kld_stop_dev(bpf_engine* e, const void* window_dev, int stride, int n_keys, int* handled_out,
                     int* stop_count_out, int* leaf_count_out, int* bin_count_out);
int bpf_kld_leaf_count(bpf_engine* e, int* leaf_count_out, int* bin_count_out);

/* ------------------------------------------------------------------ wire formats
 * The callers' data shaping, as plain host functions (no engine needed). */
/* Node2D::updateLatestScanData (node_2d.cpp:531-560): float LaserScan ranges -> PlanarData.
 * sensor_min_range / sensor_max_range <= 0 mean "not set".  ranges_out / angles_out hold n doubles. */
int bpf_wire_laserscan_to_planar(const float* ranges, int n, float msg_range_min, float msg_range_max,
                                 double sensor_min_range, double sensor_max_range, double angle_min,
                                 double angle_increment, double* ranges_out, double* angles_out,
                                 double* range_max_out);
/* Node2D::getAngleStats (node_2d.cpp:497-529): first bearing and bearing increment of a scanner in the base
 * frame (an upside-down scanner gets a negative increment).  q_base_from_scanner = rotation (x, y, z, w)
 * of the base_frame <- scan frame transform the node looks up.  Quaternion helpers are third-party tf2
 * (setRPY, operator*, getYaw), restated from their published form. */
int bpf_wire_scan_angle_stats(double msg_angle_min, double msg_angle_increment, const double q_base_from_scanner[4],
                              double* angle_min_out, double* angle_increment_out);
/* Node2D::convertMap (node_2d.cpp:265-295): nav_msgs/OccupancyGrid -> tri-state cells with integer
 * up-scaling and the centre origin (narrowed to float like pcl::PointXYZ).  cells_out holds
 * (width*scale) * (height*scale) int32. */
int bpf_wire_occupancy_grid_to_cells(const int8_t* data, int width, int height, double msg_resolution,
                                     double msg_origin_x, double msg_origin_y, int map_scale_up_factor,
                                     int32_t* cells_out, int* size_x_out, int* size_y_out, float origin_out[2],
                                     double* resolution_out);
/* Node3D::updateLatestScanData (node_3d.cpp:467-480): keep every step-th point, step = max((n-1)/(max_beams-1), 1).
 * Returns the number of points written (xyz triples); capacity in points. */
int bpf_wire_decimate_cloud(const float* points_xyz, int n_points, int max_beams, float* out_xyz, int capacity);
/* Node::publishParticleCloud (node.cpp:335-357): samples -> PoseArray entries {x, y, 0, qx, qy, qz, qw}
 * with q = setRPY(0, 0, theta). */
int bpf_wire_samples_to_pose_array(const double* samples, int sample_count, double* poses7_out);

/* ------------------------------------------------------------------ exhaustive pose search
 * Global localisation without the lottery of random trial poses: every free cell of the 2-D map at every one of
 * `headings` headings is scored against one scan, and the best k candidates come back.  NOT a reference call (parity
 * unpinned by construction); the score is the one BPF_POSE_CHECK_SENSOR_MODEL uses.
 *
 * Free list F: Node2D::updateFreeSpaceIndices for the current map and the non_free_space_radius of
 * bpf_planar_set_map_factors (FREE cells whose LUT distance, compared in double, is > radius; i outer, j inner).
 * cell_stride s >= 1 keeps the entries with i % s == 0 && j % s == 0, in the same order: F_s.
 * Candidate c in [0, |F_s| * headings) is cell f = c / headings at heading h = c % headings, with the pose
 *   x = origin_x + (i - size_x / 2) * resolution, y = origin_y + (j - size_y / 2) * resolution   (integer halves),
 *   theta = (2.0 * pi * h) / headings - pi   (pi = 3.14159265358979323846, evaluated in double as written).
 * Its score is the weight of the one-sample set {pose, 1.0} after PlanarScanner::applyModelToSampleSet with
 * set->converged = 0 (no beam skipping) against the scan given here, under the planar model, map factors and scanner
 * pose configured on the engine; with max_beams < 2 that is 1.0.  Status codes of the scoring path pass through
 * (BPF_ERR_BEAM_STEP, BPF_ERR_NOT_CONFIGURED ...).
 *
 * Result: the best min(k, count) candidates of [first, first + count), by score descending, equal scores by
 * candidate ascending; a NaN score ranks below every number.  count = -1: to the end of the space.
 * Limits: 1 <= k <= 1024, headings >= 1, cell_stride >= 1 and first / count inside the space, otherwise
 * BPF_ERR_INVALID_ARGUMENT; |F_s| * headings > 2^31 - 1 returns BPF_ERR_CAPACITY before anything is launched.
 * A map without a free cell beyond the radius gives *n_hits_out = 0 and BPF_OK.
 *
 * The call needs the 2-D map, its LUT and a planar model (BPF_ERR_NOT_CONFIGURED without them, also when only the
 * cloud scanner is configured); it needs no filter and leaves one as it found it: sets, weights and the caches
 * behind them, the drand48 state, w_slow / w_fast, the beam-skip working data, the scan remembered for the pose
 * check, last_status and the lazy statistics.  Candidates are generated, scored and selected on the device in
 * windows of bpf_pose_search_window() candidates, all enqueued back to back; the host waits once. */
typedef struct
{
  double pose[3];      /* x, y, theta of the candidate */
  double score;
  long long candidate; /* c */
  int i, j;            /* its map cell */
  int heading;         /* h */
  int reserved;
} bpf_pose_hit;

int bpf_planar_search_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                            double range_max, int headings, int cell_stride, long long first, long long count,
                            int k, bpf_pose_hit* hits_out, int* n_hits_out);
/* |F_s| * headings for the current map and radius: what a caller splits into ranges (the product itself, also when
 * it is past the limit of a search) */
int bpf_planar_search_space(bpf_engine* e, int headings, int cell_stride, long long* candidates_out,
                            int* free_cells_out);
/* merges hit lists of disjoint ranges (n_lists lists back to back in `lists`, list_lengths[l] rows each) into the
 * best k, same order rule; plain host code, needs no engine */
int bpf_pose_search_merge(const bpf_pose_hit* lists, const int* list_lengths, int n_lists, int k,
                          bpf_pose_hit* hits_out, int* n_hits_out);
/* candidates scored per window, an internal constant the tests size their cases from; needs no engine */
int bpf_pose_search_window(void);

/* The same search, pruned: the rows of bpf_planar_search_poses, bit for bit, from fewer exact evaluations.  NOT a
 * reference call.  Likelihood field and likelihood-field Gompertz only.
 *
 * block B (one of 2, 4, 8, 16, 32, 64) cuts the map into B x B blocks of cells: block (bi, bj) holds the cells with
 * i / B == bi and j / B == bj.  The block list holds the blocks with at least one entry of F_s, bi outer, bj inner.
 * Block candidate q = block_index * headings + h stands for the candidates c = f * headings + h of the exhaustive
 * search whose cell F_s[f] lies in the block (its members); numbering, poses and scores of the candidates are those
 * of bpf_planar_search_poses.  The bound of q is the block's anchor pose -- the cell (bi * B, bj * B), free or not,
 * at heading h -- scored by the same scoring path against a min-pooled copy of the LUT image, with neutral map
 * factors, times max(1, off_map_factor, non_free_factor); for Gompertz a small margin is added.  bound(q) >=
 * score(c), as doubles, for every member c ("Pose search, pruned form").
 *
 * The call scores every bound, then the members of the min(1024, count) block candidates of the best bounds exactly
 * (the seed, as large as the bound list whatever k is); tau is the k-th best exact score once k are known.  A block
 * candidate with bound < tau is never expanded; the others are, in windows of at most bpf_pose_search_window()
 * members, each checked once more against the tau of that moment.  A NaN bound is never pruned; equal scores keep
 * their order by candidate.  The host waits twice: once for the number of surviving block candidates, once for the
 * rows.
 *
 * first_block / block_count select a range of the block list (block_count = -1: to its end), so that a sharded
 * caller can split the space; lists of disjoint ranges merge with bpf_pose_search_merge.
 *
 * Status: BPF_ERR_UNSUPPORTED, before anything is launched, for the prob and beam models, for a Gompertz whose a, b,
 * c or input_scale is not > 0, for map factors that are negative or NaN, and for a per-level term table that is not
 * non-increasing over levels 0 .. K.  BPF_ERR_INVALID_ARGUMENT for a block that is not in the list, a range outside
 * the block list, and what bpf_planar_search_poses refuses.  BPF_ERR_CAPACITY for |F_s| * headings > 2^31 - 1 and
 * for more than 2^24 block candidates in one call (18 bytes of device memory each, about 300 MB at the limit; split
 * the range, or raise block).  With max_beams < 2 every score is 1.0, as in the exhaustive call.  Read-only for the
 * filter, exactly as bpf_planar_search_poses is. */
typedef struct
{
  long long candidates;               /* what bpf_planar_search_poses would score for the same range */
  long long block_candidates;         /* = seed_candidates + pruned_block_candidates + expanded_block_candidates */
  long long seed_candidates;          /* block candidates expanded as the seed */
  long long pruned_block_candidates;  /* never expanded: below tau behind the seed, or at their window */
  long long expanded_block_candidates;
  long long scored_candidates;        /* exact evaluations: members of the seed and of the expanded */
  long long windows;                  /* scoring launches of the call: bound, seed and expansion windows */
} bpf_pose_search_stats;

int bpf_planar_search_poses_pruned(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                   double range_max, int headings, int cell_stride, int block, int first_block,
                                   int block_count, int k, bpf_pose_hit* hits_out, int* n_hits_out,
                                   bpf_pose_search_stats* stats_out /* nullable */);
/* number of blocks in the block list of (cell_stride, block) for the current map and radius */
int bpf_planar_search_blocks(bpf_engine* e, int cell_stride, int block, int* n_blocks_out);
/* the pooled image P_B of the current map as the bound pass reads it: ltx * lty tiles of 64 u16 codes (level * 8),
 * the layout of the engine's LUT image.  *n_out = entries of the image; tiles_out may be null to ask for the size
 * alone, otherwise capacity >= *n_out entries.  For diagnosis and for the tests. */
int bpf_planar_search_pooled_lut(bpf_engine* e, int block, unsigned short* tiles_out, long long capacity,
                                 long long* n_out, int* ltx_out, int* lty_out);
/* the bounds the pruning uses, as doubles, of the block candidates first_q .. first_q + count - 1 (q over the whole
 * block list; count = -1: to the end).  For diagnosis and for the tests; refusals as above. */
int bpf_planar_search_bounds(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                             double range_max, int headings, int cell_stride, int block, long long first_q,
                             long long count, double* bounds_out);

/* The same search with the 3-D map and the cloud scanner: Node3D's global localisation without the lottery over the
 * columns of the map's bounding rectangle.  NOT a reference call (parity unpinned by construction).
 *
 * Column list C: Node3D::updateFreeSpaceIndices (node_3d.cpp:306-318) for the current 3-D map -- every column (i, j)
 * with min_i <= i < max_i and min_j <= j < max_j of its cell bounds, i outer, j inner.  cell_stride s >= 1 keeps the
 * columns whose i and j are both divisible by s (the bounds may be negative: i0 = the first multiple of s that is
 * >= min_i, likewise j0), in the same order: C_s, n_i x n_j columns.  C_s is arithmetic, never a list.
 * Candidate c in [0, |C_s| * headings) is column f = c / headings at heading h = c % headings, with
 *   (i, j) = (i0 + (f / n_j) * s, j0 + (f % n_j) * s),
 *   x = i * resolution, y = j * resolution   (OctoMap::convertMapToWorld, octomap.cpp:83-95: one double multiply each),
 *   theta = (2.0 * pi * h) / headings - pi   (pi = 3.14159265358979323846, evaluated in double as written).
 * Its score is the weight of the one-sample set {pose, 1.0} after PointCloudScanner::applyModelToSampleSet against
 * the n_points packed float xyz triples given here -- exactly what bpf_cloud_apply_model_to_sample_set returns for
 * that sample --, under the cloud model, off_map_factor and scanner-to-footprint tf configured on the engine; with
 * cloud max_beams < 2 that is 1.0.  The points are taken as given: decimation (bpf_wire_decimate_cloud) stays with the
 * caller, as at bpf_cloud_apply_model_to_sample_set.
 *
 * Result: the best min(k, count) candidates of [first, first + count), by score descending, equal scores by
 * candidate ascending; a NaN score ranks below every number.  count = -1: to the end of the space.  The rows are
 * bpf_pose_hit (i, j = the column's cell indices); lists of disjoint ranges merge with bpf_pose_search_merge.
 * Limits: a cloud and the outputs non-null, n_points >= 1, 1 <= k <= 1024, headings >= 1, cell_stride >= 1 and
 * first / count inside the space, otherwise BPF_ERR_INVALID_ARGUMENT; |C_s| * headings > 2^31 - 1 returns
 * BPF_ERR_CAPACITY before anything is launched.  Bounds or a stride that leave no column give *n_hits_out = 0 and
 * BPF_OK.
 *
 * The call needs the 3-D map and a cloud model (BPF_ERR_NOT_CONFIGURED without them, also when only the planar scanner
 * is configured); it needs no filter and leaves one as it found it: sets, weights and the caches behind them, the
 * drand48 state, w_slow / w_fast, the scan remembered for the pose check, the lazy statistics, and what describes the
 * engine's last scoring call (evaluations, bpf_cloud_last_form, last_status, the profile: the search's launches are
 * not timed).  The cloud and the term table are staged once per call; candidates are generated, scored and selected on
 * the device in windows of bpf_pose_search_window() candidates, all enqueued back to back; the host waits once before
 * the first launch (for the staging buffers) and once for the rows. */
int bpf_cloud_search_poses(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                           long long first, long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out);
/* |C_s| * headings for the current 3-D map (needs the map only): what a caller splits into ranges (the product
 * itself, also when it is past the limit of a search); *columns_out = |C_s| */
int bpf_cloud_search_space(bpf_engine* e, int headings, int cell_stride, long long* candidates_out, int* columns_out);

/* ------------------------------------------------------------------ joint pose search over several scans
 * One scan cannot tell the look-alike poses of a periodic environment apart; the last few scans with the odometry
 * between them, or two sensors at a known rigid offset, can.  Every candidate of bpf_planar_search_poses /
 * bpf_cloud_search_poses is scored against n_scans scans, scan s taken at the candidate's pose composed with a rigid
 * offset D_s, and the best k come back.  NOT reference calls (parity unpinned by construction).
 *
 * Scans: 1 <= n_scans <= 16.  Planar: scan s is (ranges[s], angles[s], range_counts[s], range_maxes[s]); counts and
 * range_max may differ between scans.  Cloud: scan s is n_points[s] packed float xyz triples at points_xyz[s], taken as
 * given; sizes may differ.
 * Offsets: offsets[3 * s ...] = D_s = (dx, dy, dth), finite doubles: the robot's pose at scan s expressed in the frame
 * of the candidate pose (an odometry delta; for a second sensor, the offset that makes pose (+) D_s (+) scanner_pose
 * that sensor's pose).  D_0 need not be zero.
 * Candidates: enumeration, numbering, first / count, count = -1, k <= 1024 and the 2^31 - 1 limit are those of the
 * single-scan calls; candidate c has the base pose (x, y, theta_h) they give it.  In addition headings <= 65536
 * (BPF_ERR_CAPACITY otherwise), because of the table below.
 * Composed pose, as coordAdd writes it (planar_scanner.cpp:693-701), left to right, no contraction:
 *   x_s = (x + dx * C_h) - dy * S_h,  y_s = (y + dx * S_h) + dy * C_h,  theta_s = theta_h + dth   (not normalised: the
 *   scoring path normalises where the reference does)
 * with C_h = cos(theta_h), S_h = sin(theta_h) from a table of `headings` entries that the host fills with the C
 * library's cos / sin of the double theta_h, once per call: bpf_pose_search_heading_table gives the same table.  So a
 * composed pose is bit for bit what a host model computes with the same libm.
 * Joint score: w_0 = 1.0; w_{s+1} is the weight of the one-sample set {(x_s, y_s, theta_s), w_s} after
 * applyModelToSampleSet (set->converged = 0) against scan s, under the model, map factors / off_map_factor and scanner
 * pose / tf configured on the engine; the score is w_S: the un-normalised weight that a noise-free particle started at
 * the candidate carries after the S sensor updates.  It is NOT the product of S separately rounded single-scan
 * scores.  With max_beams < 2 every score is 1.0.
 * Result: bpf_pose_hit rows in the order of the single-scan calls; `pose` is the BASE pose of the candidate, i, j,
 * heading and candidate as there.  Lists of disjoint ranges merge with bpf_pose_search_merge.
 *
 * Status: BPF_ERR_INVALID_ARGUMENT for n_scans outside 1 .. 16, a non-finite offset, a null scan or output, a scan
 * with range_count / n_points <= 0, and what the single-scan calls refuse; BPF_ERR_NOT_CONFIGURED without map / LUT /
 * model; BPF_ERR_CAPACITY as above; the scoring path's own codes pass through.  Read-only for a filter, exactly as the
 * single-scan searches are.  Per window of bpf_pose_search_window() candidates the device runs, for every scan, the
 * composition and the scoring path, then one selection; the host waits where the single-scan searches wait (the
 * planar form stages a scan per scoring call, so with n_scans >= 4 it also waits at the staging ring). */
/* cos / sin of theta_h = (2.0 * pi * h) / headings - pi, h = 0 .. headings - 1, as the joint calls tabulate them;
 * 1 <= headings <= 65536; needs no engine */
int bpf_pose_search_heading_table(int headings, double* cos_out, double* sin_out);
int bpf_planar_search_poses_joint(bpf_engine* e, int n_scans, const double* const* ranges,
                                  const double* const* angles, const int* range_counts, const double* range_maxes,
                                  const double* offsets /* [n_scans][3] */, int headings, int cell_stride,
                                  long long first, long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out);
int bpf_cloud_search_poses_joint(bpf_engine* e, int n_scans, const float* const* points_xyz, const int* n_points,
                                 const double* offsets /* [n_scans][3] */, int headings, int cell_stride,
                                 long long first, long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out);
/* Diagnostic: the n_scans composed poses of the n candidates given (any order, repeats allowed), formed by the joint
 * search's own kernel: poses_out[n][n_scans][3].  Needs the map of the space only (and its LUT, planar); a candidate
 * outside the space is BPF_ERR_INVALID_ARGUMENT. */
int bpf_planar_search_joint_poses(bpf_engine* e, int headings, int cell_stride, const double* offsets, int n_scans,
                                  const long long* candidates, int n, double* poses_out);
int bpf_cloud_search_joint_poses(bpf_engine* e, int headings, int cell_stride, const double* offsets, int n_scans,
                                 const long long* candidates, int n, double* poses_out);

/* The cloud search, pruned: the rows of bpf_cloud_search_poses, bit for bit, from fewer exact evaluations.  NOT a
 * reference call.  The structure, the stats and their invariants are those of bpf_planar_search_poses_pruned.
 *
 * block B (one of 2, 4, 8, 16, 32, 64): block (bi, bj) holds the columns of C_s with floor(i / B) == bi and
 * floor(j / B) == bj (floor division: the cell bounds may be negative).  The block list holds the blocks with at
 * least one column of C_s, bi outer, bj inner; it is the product of two per-axis lists, never a per-column list.
 * Block candidate q = block_index * headings + h stands for the candidates c = f * headings + h of
 * bpf_cloud_search_poses whose column lies in the block; numbering, poses and scores are unchanged.  The bound of q
 * is the anchor pose -- the column (bi * B, bj * B), inside the rectangle or not, x = i * resolution, y = j *
 * resolution, at heading h -- scored by the same scoring launches against the pooled volume P_B with off_map_factor
 * taken as 1, times max(1, off_map_factor) (min(1, ...) under a negative value); for Gompertz a small margin is
 * added first.  P_B has the layout of the engine's dense volume; its entry at grid position (x, y) of plane k is the
 * smallest distance ratio of the on-map cells of the window [x - 1, x + B] x [y - 1, y + B] of that plane (the far
 * border entry: of the cells within B + 1 of either edge), the border code when there is none.  bound(q) >=
 * score(c), as doubles, for every member c ("Pose search, pruned 3-D form").
 *
 * Seed, tau, survivors, expansion and the two waits behind the staging are as in the planar call; first_block /
 * block_count select a range of the block list (block_count = -1: to its end), and lists of disjoint ranges merge
 * with bpf_pose_search_merge.
 *
 * Status: BPF_ERR_NOT_CONFIGURED without the 3-D map or a cloud model.  BPF_ERR_UNSUPPORTED, before any scoring
 * launch: a scanner mounting with roll or pitch; a 3-D map without the dense volume or with fewer than two distance
 * ratios free for the border codes (or BPF_OPT_CLOUD_DENSE off); a Gompertz whose a, b, c or input_scale is not > 0;
 * an off_map_factor that is negative or NaN; a term table that is not non-increasing over the ratios 0 .. 255 and
 * the off-map term; a cloud too large for the resolution -- with L = the largest |x| + |y| over the points whose
 * coordinates are all finite, + |tf_x| + |tf_y| + (the largest |cell bound| in x, y + B) * resolution, the call needs
 * L * 2^-21 < resolution (points with a non-finite coordinate are off the map at every pose and do not count).
 * BPF_ERR_INVALID_ARGUMENT for a block that is not in the list, a range outside the block list and what
 * bpf_cloud_search_poses refuses.  BPF_ERR_CAPACITY for |C_s| * headings > 2^31 - 1, more than 2^24 block candidates
 * in one call and more than 2^26 blocks.  P_B takes as much device memory as the dense volume (up to 1 GiB) per block
 * size used, reserved on first use; when that fails the call returns the allocation's error.  With cloud max_beams < 2
 * every score is 1.0.  Read-only for the filter, exactly as bpf_cloud_search_poses is. */
int bpf_cloud_search_poses_pruned(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                                  int block, int first_block, int block_count, int k, bpf_pose_hit* hits_out,
                                  int* n_hits_out, bpf_pose_search_stats* stats_out /* nullable */);
/* number of blocks in the block list of (cell_stride, block) for the current 3-D map (needs the map only) */
int bpf_cloud_search_blocks(bpf_engine* e, int cell_stride, int block, int* n_blocks_out);
/* the pooled volume P_B of the current 3-D map as the bound pass reads it: *planes_out planes (the map's z cells and
 * the zero plane behind them) of *ntx_out x *nty_out tiles of 64 bytes, the layout of the engine's dense volume.
 * *n_out = bytes of the volume; bytes_out may be null to ask for the size and the geometry alone, otherwise capacity
 * >= *n_out.  BPF_ERR_UNSUPPORTED without the dense volume or the border codes.  For diagnosis and for the tests. */
int bpf_cloud_search_pooled_lut(bpf_engine* e, int block, unsigned char* bytes_out, long long capacity,
                                long long* n_out, int* ntx_out, int* nty_out, int* planes_out);
/* the bounds the pruning uses, as doubles, of the block candidates first_q .. first_q + count - 1 (q over the whole
 * block list; count = -1: to the end).  For diagnosis and for the tests; refusals as above. */
int bpf_cloud_search_bounds(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                            int block, long long first_q, long long count, double* bounds_out);

/* ------------------------------------------------------------------ pose search over a sharded filter
 * The four searches above as one collective call each: every rank of a connected world (bpf_shard_bootstrap,
 * bpf_shard_mailbox_connect or bpf_shard_connect_local) calls with the SAME arguments and the same scan or cloud, and
 * every rank returns the same rows -- the single engine's rows for that range, byte for byte.  NOT reference calls.
 *
 * Split.  The range given has T units (candidates for the exhaustive forms, blocks for the pruned ones; count /
 * block_count = -1: to the end); rank r of W takes units [first + T r / W, first + T (r + 1) / W) in integer
 * arithmetic.  A rank whose share is empty scores nothing and contributes an empty list.
 * Merge.  A rank's best-k list stays on the device; it crosses between the ranks as 16 bytes per row (k rows and a
 * header, over the engine's exchange), the W lists are folded into the best k on every rank's device in the order of
 * the single-engine search (score descending, equal scores by candidate, NaN last), and only the k rows come down.
 * Shared tau (pruned forms).  Behind its seed stage every rank publishes the key of the k-th score of its exact list
 * (0 while the list is short or that score is a NaN); the largest of the W words is a floor under every rank's tau
 * from then on.  The global k-th best score is at least every rank's tau, so a block candidate whose bound is
 * strictly below the floor holds no row of the result.  A rank's OWN list is then no longer the best k of its range:
 * only the merged rows are a result, and stats_out (this rank's counters, for this rank's share) depends on the
 * other ranks' seeds.
 *
 * Everything the single-engine call refuses from its arguments and the configuration is refused before the first
 * exchange, by every rank alike; the limit of 2^31 - 1 candidates applies to the whole space, the limit of 2^24 block
 * candidates to each rank's share.  BPF_ERR_NOT_CONFIGURED without a connected world; BPF_ERR_CAPACITY when the
 * mailbox's window region is smaller than W * (2 k + 2) words.  Read-only for the filter on every rank, as the
 * single-engine searches are.  Nothing of this has run between two GPUs: what the split buys is counted in
 * evaluations and bytes (profiles/pose_search_sharded.md), not measured as a speed-up. */
int bpf_shard_search_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                           double range_max, int headings, int cell_stride, long long first, long long count, int k,
                           bpf_pose_hit* hits_out, int* n_hits_out);
int bpf_shard_search_poses_pruned(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                                  double range_max, int headings, int cell_stride, int block, int first_block,
                                  int block_count, int k, bpf_pose_hit* hits_out, int* n_hits_out,
                                  bpf_pose_search_stats* stats_out /* nullable */);
int bpf_shard_cloud_search_poses(bpf_engine* e, const float* points_xyz, int n_points, int headings, int cell_stride,
                                 long long first, long long count, int k, bpf_pose_hit* hits_out, int* n_hits_out);
int bpf_shard_cloud_search_poses_pruned(bpf_engine* e, const float* points_xyz, int n_points, int headings,
                                        int cell_stride, int block, int first_block, int block_count, int k,
                                        bpf_pose_hit* hits_out, int* n_hits_out,
                                        bpf_pose_search_stats* stats_out /* nullable */);

/* ------------------------------------------------------------------ pose refinement
 * Sub-cell, sub-degree poses from the hits of a search (or from any poses): a coarse-to-fine descent on a lattice
 * around each pose, all of it on the device.  NOT a reference call (parity unpinned by construction).
 *
 * R = xy_radius, A = theta_radius, L = levels.  The lattice has M = (2R+1)^2 (2A+1) points; point m is
 * (a (2R+1) + b) (2A+1) + t with a, b in [0, 2R] and t in [0, 2A]; the centre m_c has a = b = R, t = A.
 * At level l in [0, L) the steps are d_l = xy_step * 2^-l and q_l = theta_step * 2^-l (ldexp: exact), and the pose
 * of point m around the centre (cx, cy, ctheta) is, evaluated in double as written with no contraction,
 *   x = cx + (double)(a - R) * d_l,  y = cy + (double)(b - R) * d_l,  theta = ctheta + (double)(t - A) * q_l.
 * A step whose radius is 0 is not read (it counts as 0.0).  The score of a pose is exactly the search's: the weight
 * of the one-sample set {pose, 1.0} after applyModelToSampleSet with set->converged = 0 (planar form) or what
 * bpf_cloud_apply_model_to_sample_set returns for it (cloud form), under the model, map factors and scanner pose /
 * tf configured on the engine; 1.0 with max_beams < 2.
 *
 * The new centre is the best point of the lattice: score descending; among equal scores the centre before every
 * other point, then m ascending; NaN below every number.  A centre chosen again is not rewritten, so a flat or
 * all-NaN neighbourhood leaves the pose bit for bit where it was.  Level l + 1 starts from level l's centre, level 0
 * from the input pose.  Row r of `out` refines pose r (the input order is kept; the caller sorts); trace_out, when
 * not NULL, receives n_poses * levels ints, trace_out[r * L + l] = the m chosen for pose r at level l.
 *
 * Limits: 1 <= n_poses <= 1024, R >= 0, A >= 0, 2 <= M <= 2048, 1 <= L <= 16, xy_step finite and > 0 when R > 0,
 * theta_step finite and > 0 when A > 0, every input pose finite, the scan (cloud), poses_xyt and out non-null,
 * otherwise BPF_ERR_INVALID_ARGUMENT.  Requirements and the status codes of the scoring path are those of the matching
 * search call (BPF_ERR_NOT_CONFIGURED, BPF_ERR_BEAM_STEP ...).
 *
 * Like the searches the call needs no filter and leaves one as it found it (the same state is saved and put back).
 * Poses are processed in groups of max(1, bpf_pose_search_window() / M), so that a launch scores at most one window
 * of candidates; the result does not depend on the grouping.  All levels of all groups are enqueued back to back;
 * the host waits once for the rows (the cloud form once more before its first launch, for the staging buffers). */
typedef struct
{
  double pose[3];  /* refined x, y, theta (theta as accumulated, NOT normalised) */
  double score;    /* score of `pose`, from the level that chose it last */
  double score_in; /* score of the input pose (the centre of level 0) */
  int moved;       /* number of levels at which the centre changed (the chosen m was not m_c) */
  int reserved;    /* 0 */
} bpf_pose_refined; /* 48 bytes in every binding */

int bpf_planar_refine_poses(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                            double range_max, const double* poses_xyt, int n_poses, int xy_radius, double xy_step,
                            int theta_radius, double theta_step, int levels, bpf_pose_refined* out, int* trace_out);
int bpf_cloud_refine_poses(bpf_engine* e, const float* points_xyz, int n_points, const double* poses_xyt, int n_poses,
                           int xy_radius, double xy_step, int theta_radius, double theta_step, int levels,
                           bpf_pose_refined* out, int* trace_out);
/* M and m_c of a lattice (either output may be NULL); BPF_ERR_INVALID_ARGUMENT for a negative radius, M < 2 or
 * M > 2048.  Plain host code, needs no engine */
int bpf_pose_refine_lattice(int xy_radius, int theta_radius, int* points_out, int* centre_out);

/* ------------------------------------------------------------------ from hit rows to mixture components
 * The step between the searches / refinements above and bpf_pf_init_with_mixture.  Not a reference call.  Plain host
 * code, needs no engine.  poses_xyt = n_rows x (x, y, theta), scores = n_rows (search hits and refined rows alike).
 *  1. Rows with a non-finite pose or a score that is NaN, infinite or <= 0 are dropped; the rest are taken by score
 *     descending, equal scores by row index ascending.
 *  2. A row is suppressed by an already kept component c when |x - x_c| <= xy_merge, |y - y_c| <= xy_merge and
 *     |normalize_angle(theta - theta_c)| <= theta_merge (x_c, y_c, theta_c: the kept ROW's values; normalize_angle in
 *     the fmod form, no trigonometry); it increments merged_out[c].  Any other row becomes a component until
 *     max_components are kept; later unsuppressed rows are dropped.
 *  3. Component k: x, y copied bit for bit, theta = normalize_angle(theta) (refined theta comes accumulated),
 *     rotation the identity, sigma as given, source_row_out[k] its row.
 *  4. Counts by largest remainder on the scores: W = sum of the kept scores in component order,
 *     t_k = ((double)total_count * score_k) / W, c_k = floor(t_k); the samples left over go one each to the components
 *     by t_k - c_k descending (equal remainders by k ascending), wrapping round; should rounding make the floors
 *     exceed total_count, one is taken from the components that have any in the reverse of that order until it fits.
 *     The counts sum to total_count exactly; components with count 0 can appear.
 * out holds max_components entries, source_row_out / merged_out (either may be NULL) max_components ints.
 * BPF_ERR_INVALID_ARGUMENT: a NULL array, n_rows or max_components outside [1, 1024], total_count < 1, a negative or
 * non-finite merge distance or sigma, no usable row. */
int bpf_pose_mixture_from_hits(const double* poses_xyt, const double* scores, int n_rows, int total_count,
                               double xy_merge, double theta_merge, int max_components, const double sigma[3],
                               bpf_mixture_component* out, int* source_row_out, int* merged_out,
                               int* n_components_out);

/* ------------------------------------------------------------------ pose moments
 * The shape of the score surface around a pose (a refined hit, usually): score-weighted first and second moments of
 * ONE lattice per pose, all of it on the device.  NOT a reference call (parity unpinned by construction).
 *
 * Lattice, point numbering, pose expressions and scores are those of level 0 of the refinement above, with
 * d = xy_step and q = theta_step as given (a step whose radius is 0 is not read and counts as 0.0); 1.0 everywhere
 * with max_beams < 2.  With s_m the score of point m, in double, no contraction, evaluated as written:
 *   s_max = the largest s_m, NaN below every number (NaN when no s_m is a number); the argmax is the refinement's
 *           (the centre first among equal scores, then m ascending);
 *   thr = baseline * s_max;  w_m = s_m - thr when s_m > thr, else 0 (NaN gives 0);
 *   da = (double)(a - R), db = (double)(b - R), dt = (double)(t - A);
 *   W = sum w;  Sa = sum w*da (Sb, St alike);  Saa = sum (w*da)*da (Sab, Sat, Sbb, Sbt, Stt alike: (w*du)*dv);
 *   ma = Sa / W (mb, mt alike);  mean = (cx + ma*d, cy + mb*d, ctheta + mt*q);
 *   cov_uv = ((Suv / W - mu*mv) * step_u) * step_v   with step_a = step_b = d, step_t = q.
 * The ten sums are formed in a fixed order: 256 partial sums, partial p adding its points m = p, p + 256, ...
 * ascending from 0.0; within each 64 consecutive partials the xor butterfly v = v + v[lane ^ off] with off = 32, 16,
 * ..., 1; then the four results added in the order 0, 1, 2, 3.
 * A row is valid iff s_max is a number and > 0 (then W >= (1 - baseline) * s_max > 0).  An invalid row has flags = 0,
 * support = 0, weight_sum and cov 0.0 and the mean equal to the input pose bit for bit; score_max stays s_max (the
 * canonical quiet NaN 0x7ff8000000000000 when no score is a number).
 *
 * scores_out, when not NULL, receives the n_poses * M lattice scores, scores_out[r * M + m].
 * Limits and refusals are the refinement's (1..1024 poses, 2 <= M <= 2048, finite poses, the step rules, the
 * BPF_ERR_NOT_CONFIGURED cases of the matching refine call) and 0 <= baseline < 1, finite; every refusal happens before
 * anything is launched.  Read-only for a filter, like the refinement; poses are processed in groups of
 * max(1, bpf_pose_search_window() / M), the result does not depend on the grouping, and the host waits once for the
 * rows (the cloud form once more before its first launch, for the staging buffers). */
typedef struct
{
  double mean[3];    /* x, y, theta (theta accumulated, not normalised) */
  double cov[6];     /* xx, xy, xt, yy, yt, tt */
  double weight_sum; /* W */
  double score_max;  /* s_max; NaN when no lattice score is a number */
  int support;       /* lattice points with w > 0 */
  int flags;         /* bit 0: valid; bits 1..3: argmax on the lattice's outer face in x / y / theta (radius > 0 only) */
} bpf_pose_moments;  /* 96 bytes in every binding */
enum
{
  BPF_MOMENTS_VALID = 1,
  BPF_MOMENTS_FACE_X = 2,
  BPF_MOMENTS_FACE_Y = 4,
  BPF_MOMENTS_FACE_THETA = 8
};

int bpf_planar_pose_moments(bpf_engine* e, const double* ranges, const double* angles, int range_count,
                            double range_max, const double* poses_xyt, int n_poses, int xy_radius, double xy_step,
                            int theta_radius, double theta_step, double baseline, bpf_pose_moments* out,
                            double* scores_out);
int bpf_cloud_pose_moments(bpf_engine* e, const float* points_xyz, int n_points, const double* poses_xyt, int n_poses,
                           int xy_radius, double xy_step, int theta_radius, double theta_step, double baseline,
                           bpf_pose_moments* out, double* scores_out);

/* Moments to the rotation / sigma of mixture components.  Plain host code, needs no engine.  Component k takes row
 * r = source_row[k]; a component whose row is invalid keeps what it had.  For a valid row:
 *  - the symmetric 3 x 3 cov goes through cyclic Jacobi: pairs (0,1), (0,2), (1,2) per sweep, a rotation skipped when
 *    the off-diagonal entry is exactly 0, at most 8 sweeps, stopping early when all three off-diagonal entries are 0;
 *    tau = (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| + sqrt(tau^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c; only
 *    + - * / and sqrt, no contraction; eigenvalues stay in diagonal order (not sorted);
 *  - rotation = the eigenvectors as columns, row-major (the cr_ of bpf_pf_init_with_gaussian);
 *  - sigma[i] = sqrt(lambda_i clamped to [floor_j^2, cap_j^2]) with j the axis (x, y, theta) on which eigenvector i
 *    has its largest absolute entry, the lowest axis winning ties;
 *  - take_mean != 0: mean = the moments' mean, theta normalised (fmod form); otherwise the mean is untouched;
 *  - count is untouched.
 * BPF_ERR_INVALID_ARGUMENT: a NULL array, n_components or n_rows outside [1, 1024], a source_row entry outside
 * [0, n_rows), a negative or non-finite floor or cap, cap < floor, a non-finite cov in a valid row (used by a
 * component or not); nothing is written then. */
int bpf_pose_mixture_apply_moments(bpf_mixture_component* comps, int n_components, const int* source_row,
                                   const bpf_pose_moments* rows, int n_rows, const double sigma_floor[3],
                                   const double sigma_cap[3], int take_mean);

/* ------------------------------------------------------------------ measurement */
/* free / total device memory as hipMemGetInfo reports it (diagnostic; used by the leak test) */
int bpf_device_memory_info(int device_ordinal, size_t* free_bytes, size_t* total_bytes);
enum
{
  BPF_K_SCORE = 0,     /* sensor scoring kernel, gather form (k_score_field / k_score_beam / k_cloud_score) */
  BPF_K_REDUCE = 1,
  BPF_K_NORMALIZE = 2,
  BPF_K_CDF = 3,
  BPF_K_DRAW = 4,
  BPF_K_FINALIZE = 5,
  BPF_K_SCORE_WINDOW = 6, /* sensor scoring kernel, LDS-window form (k_score_window) */
  BPF_K_SCORE_AUX = 7,    /* its helpers: k_field_prep, k_field_windows, k_field_finish */
  BPF_K_MOTION = 8,       /* k_motion_* */
  BPF_K_COUNT = 9
};
typedef struct
{
  double ms[BPF_K_COUNT];          /* accumulated HIP-event time per kernel class */
  long long launches[BPF_K_COUNT];
} bpf_profile;
/* on = 1: every 8th launch of the dominant (scoring) kernel is timed by a pair of hipEvents attached to the
 * dispatch itself (hipExtLaunchKernelGGL: the kernel's own start-to-end on the engine stream, which is what the
 * rocprofv3 kernel trace reports; a timed dispatch costs the update ~5 us, hence the sampling -- `launches` counts
 * the timed ones); on = 2: every scoring launch that way and every other kernel class bracketed by hipEventRecord
 * (costs host time per event, so not for timed regions); on = 3: as 1 but EVERY scoring launch (for scoring kernels
 * of a millisecond or more, where the 5 us do not show); 0: off. */
int bpf_profile_enable(bpf_engine* e, int on);
int bpf_profile_reset(bpf_engine* e);
int bpf_profile_get(bpf_engine* e, bpf_profile* out);
/* Name of the scoring kernel as rocprofv3 prints it, for matching profiles/ summaries. */
const char* bpf_score_kernel_name(const bpf_engine* e);
/* Decision of the last likelihood-field update: *used_window = 1 when the LDS-window kernels did
 * it, with how many of the 64-beam chunks the window plan expected to cover (synchronises). */
int bpf_get_window_plan(bpf_engine* e, int* used_window, int* chunks_covered, int* chunks_total);

#ifdef __cplusplus
}
#endif
#endif /* BADGER_PF_H */
