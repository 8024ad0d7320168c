/*
 * rsreg.h — C ABI of the MI355X-native pairwise point-cloud registration engine.
 *
 * This is the drop-in boundary for the ICP / NDT pair-registration hot path of
 * hyunminch/realsense-pointcloud.  The reference has no FFI of its own; the calls that
 * cross this boundary are the PCL calls its three registration schemes make.  Every entry
 * point below names the reference call site (file:line under the reference's src/) and
 * the PCL method it stands in for.
 *
 * Conventions
 *   - Points are handed over as an array of records `stride` bytes apart whose first 12
 *     bytes are `float x, y, z` (pcl::PointXYZRGB: stride 32, rgb at byte 16).  Only xyz
 *     is ever sent to the GPU; colour stays on the host (PCL's ICP/NDT ignore it too).
 *   - 4x4 transforms are 16 floats, COLUMN-major (memcpy-compatible with Eigen::Matrix4f).
 *   - Every function returns an rsreg_status (0 = ok, < 0 = error).  Nothing throws across
 *     the ABI.  "Did not converge" is a successful call with result->converged == 0.
 *   - A ctx is bound to one device + one HIP stream and is not thread-safe; different
 *     ctxs are independent.  Host pointers are never retained after a call returns.
 *   - *_device variants take pointers to memory already resident in HBM (same record
 *     layout); the plain variants take host pointers and copy xyz up themselves.
 *   - There is NO CPU fallback: without a usable HIP device every compute entry point
 *     returns RSREG_ERR_NO_DEVICE.
 */
#ifndef RSREG_H_
#define RSREG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSREG_VERSION_MAJOR 0
#define RSREG_VERSION_MINOR 4

typedef struct rsreg_ctx rsreg_ctx;
typedef struct rsreg_cloud rsreg_cloud;   /* a cloud resident in HBM: "device-resident clouds" below */

typedef enum rsreg_status {
    RSREG_OK = 0,
    RSREG_ERR_INVALID_ARG = -1,
    RSREG_ERR_EMPTY_CLOUD = -2,
    RSREG_ERR_HIP = -3,
    RSREG_ERR_RCCL = -4,
    RSREG_ERR_NO_TARGET = -5,
    RSREG_ERR_NO_DEVICE = -6,
    RSREG_ERR_ALLOC = -7,
    RSREG_ERR_NO_SOURCE = -8,
    RSREG_ERR_STATE = -9
} rsreg_status;

/* Mirrors pcl::registration::DefaultConvergenceCriteria::ConvergenceState (same order). */
typedef enum rsreg_convergence_state {
    RSREG_CONV_NOT_CONVERGED = 0,
    RSREG_CONV_ITERATIONS = 1,
    RSREG_CONV_TRANSFORM = 2,
    RSREG_CONV_ABS_MSE = 3,
    RSREG_CONV_REL_MSE = 4,
    RSREG_CONV_NO_CORRESPONDENCES = 5,
    RSREG_CONV_FAILURE_AFTER_MAX_ITERATIONS = 6
} rsreg_convergence_state;

/* How the iteration loop decides to stop. */
typedef enum rsreg_criteria_mode {
    RSREG_CRITERIA_PCL = 0,   /* pcl DefaultConvergenceCriteria (reference behaviour)      */
    RSREG_CRITERIA_FIXED = 1  /* run exactly max_iterations iterations (benchmark mode)    */
} rsreg_criteria_mode;

/* Which kernels one ICP iteration is built from. Results are bit-identical across modes. */
typedef enum rsreg_pipeline_mode {
    RSREG_PIPELINE_STAGED = 0, /* nn_search -> cov_reduce -> transform_reject (3 kernels)   */
    RSREG_PIPELINE_FUSED = 1,  /* one fused transform+NN+reject+sums kernel per iteration  */
    RSREG_PIPELINE_DEVICE_LOOP = 2 /* FUSED, and with RSREG_CRITERIA_FIXED the 3x3 solve and the
                                  composition also run on the device: all iterations are queued
                                  without a host round trip (same arithmetic, same result);
                                  with the PCL criteria it behaves as FUSED */
} rsreg_pipeline_mode;

/* Which transformation estimate an ICP iteration solves.  RSREG_ESTIMATION_POINT_TO_PLANE_LLS is
 * pcl::IterativeClosestPointWithNormals' default (TransformationEstimationPointToPlaneLLS): it needs the target's normals
 * (rsreg_icp_set_target_normals*) and runs as RSREG_PIPELINE_STAGED whatever pipeline_mode asks for, like the correspondence
 * filters: search -> k_plane_reduce -> 6-unknown host solve -> transform.  The reference declares the point type for it and
 * never uses it (src/types.hpp:11-12).  A context whose communicator has more than one rank refuses it
 * (RSREG_ERR_INVALID_ARG from rsreg_icp_begin): the all-reduce of the 32 sums is not implemented. */
typedef enum rsreg_estimation {
    RSREG_ESTIMATION_SVD = 0,                 /* TransformationEstimationSVD (Umeyama) from the 17 sums   */
    RSREG_ESTIMATION_POINT_TO_PLANE_LLS = 1   /* the 6 x 6 linearised least squares from the 32 sums      */
} rsreg_estimation;

/*
 * ICP parameters = the setters the reference calls on pcl::IterativeClosestPoint
 *   setMaximumIterations / setMaxCorrespondenceDistance / setTransformationEpsilon /
 *   setEuclideanFitnessEpsilon — incremental_icp.hpp:46-49,
 *   icp_edge_based_registration.hpp:42-45,49-52, ndt_edge_based_registration.hpp:47-50.
 * rsreg_icp_params_default() fills PCL's defaults (10, sqrt(DBL_MAX), 0, 0, -DBL_MAX);
 * rsreg_icp_params_reference() fills the reference's constants (100, 0.01, 1, 0, 1000).
 */
typedef struct rsreg_icp_params {
    int32_t max_iterations;
    int32_t criteria_mode;                   /* rsreg_criteria_mode */
    int32_t pipeline_mode;                   /* rsreg_pipeline_mode */
    int32_t estimation;                      /* rsreg_estimation; 0 in both presets; any other value: RSREG_ERR_INVALID_ARG */
    double max_correspondence_distance;
    double transformation_epsilon;
    double transformation_rotation_epsilon;  /* <= 0: use 1 - transformation_epsilon (PCL) */
    double euclidean_fitness_epsilon;
    /* Optional correspondence filters (both off by default and in rsreg_icp_params_reference: the reference
     * constructs a CorrespondenceRejectorTrimmed and never attaches it, incremental_icp.hpp:38,
     * icp_edge_based_registration.hpp:36, ndt_edge_based_registration.hpp:33).  Either one makes the
     * iteration run as RSREG_PIPELINE_STAGED.  Both work on original records in the caller's order, also where
     * the engine merges copies of a point (sources above 65 536 points): every tie goes to the lowest index, and
     * the trim's cut can keep some copies of a point and drop others.  A context whose communicator has more
     * than one rank refuses them (RSREG_ERR_INVALID_ARG): a rank holds only its block of the source. */
    int32_t use_reciprocal_correspondences;  /* icp.setUseReciprocalCorrespondences(true): a pair (s, t) is kept only if s
                                                is also the nearest source point of t (lowest index among equidistant ones) */
    int32_t reserved1;
    double trim_overlap_ratio;               /* CorrespondenceRejectorTrimmed::setOverlapRatio(r), 0 < r < 1: of the gated
                                                pairs the floor(r * count) closest are kept, counted per source
                                                record (equal distances: lowest source index first); <= 0 or >= 1:
                                                no rejector */
} rsreg_icp_params;

/*
 * NDT parameters = the setters the reference calls on pcl::NormalDistributionsTransform
 *   setTransformationEpsilon(0.01) / setStepSize(0.1) / setResolution(1.0) /
 *   setMaximumIterations(50) — ndt_edge_based_registration.hpp:38-43.
 */
typedef struct rsreg_ndt_params {
    int32_t max_iterations;
    int32_t reserved0;
    double transformation_epsilon;
    double step_size;
    double resolution;
    double outlier_ratio;                    /* PCL default 0.55 */
} rsreg_ndt_params;

/* The 17 sums one ICP iteration reduces the correspondences to (all f64):
 *   [0] n   [1..3] sum p   [4..6] sum q   [7..15] sum q_i * p_j (row-major i,j)   [16] sum d^2
 * p = transformed source point, q = its matched target point; only pairs that pass the
 * distance gate contribute.  These are what an N-GPU run all-reduces. */
#define RSREG_NUM_SUMS 17

/* The 32 sums one POINT-TO-PLANE iteration reduces the correspondences to (all f64).  For a kept pair: p = the transformed
 * source point, q = its matched target point, n = that target record's normal (all float), W = how many source records
 * the pair stands for (exact copies are searched once; with a correspondence filter: the copies it left in play).
 * All arithmetic in double from the float inputs, every operation rounded once (no contraction):
 *   a = p x n:  a0 = n.z*p.y - n.y*p.z,  a1 = n.x*p.z - n.z*p.x,  a2 = n.y*p.x - n.x*p.y
 *   J = [a0 a1 a2 n.x n.y n.z]
 *   r = ((n.x*q.x + n.y*q.y) + n.z*q.z) - ((n.x*p.x + n.y*p.y) + n.z*p.z)
 *   a pair's terms: W * (J_i * J_j), W * (J_i * r), W * (r * r), W * (double)d2
 *   [0] sum W over the gated pairs     [1] sum W * d2, the squared distance the search returned
 *   [2] sum W over the pairs that entered the system     [3] sum W * r^2
 *   [4..24] AtA = sum W J J^T, upper triangle row-major (00 01 .. 05 11 12 .. 55)     [25..30] Atb = sum W J r     [31] 0
 * A pair whose normal has a non-finite component adds to [0] and [1] only (PCL's LLS skips it; its convergence criteria
 * still see the correspondence).  [0] and [1] are bit-equal to sums [0] and [16] of rsreg_icp_sums after the same search;
 * the order of the additions is fixed (per tile by halving over lanes, then the tiles), so the same inputs give the same
 * 32 doubles on any context, at any launch.
 * The solve (rsreg_plane_solve_from_sums, host, double): x = (alpha, beta, gamma, tx, ty, tz) = pinv(AtA) Atb by the Jacobi
 * eigen-decomposition of AtA, over the eigen-directions that carry data: eigenvalue l_k counts when
 *   l_k > ([2] + 80) * 2^-53 * trace(AtA)        (trace <= 6 l_max: relative to the largest eigenvalue, below 6 ([2] + 80) 2^-53)
 * -- a sum of N <= [2] terms, however ordered, is off by at most (N + 16) 2^-53 sum|term|; for entry (i, j) sum|term| <=
 * sqrt(AtA_ii AtA_jj) (Cauchy-Schwarz), so the error matrix has a Frobenius norm of at most ([2] + 16) 2^-53 trace(AtA), and by
 * Weyl's inequality every eigenvalue is off by no more; the other 64 units cover the eigen-solver's own rounding.  A direction
 * at or below the cut contributes nothing (the rule of the Umeyama solve: R = I where the data is silent); [2] == 0 or no
 * direction above the cut: the identity.  T = PCL's constructTransformationMatrix (1.9.1, recalled): R = Rz(gamma) Ry(beta)
 * Rx(alpha) with full sines and cosines in double, t = (tx, ty, tz), rounded to float.
 * DEVIATIONS FROM PCL 1.9.1, stated: (1) PCL accumulates AtA and Atb pair by pair in its own order, partly through float
 * intermediates; these are the sums the formulas define, in double, in the fixed order above.  (2) PCL computes
 * ATA.inverse() * ATb, which on a singular or near-singular system (one plane, parallel planes) returns whatever the
 * inverse's rounding leaves; that is not reproduced -- the pseudo-inverse above is. */
#define RSREG_NUM_PLANE_SUMS 32

typedef struct rsreg_icp_result {
    float transform[16];        /* final_transformation_, column-major                      */
    int32_t converged;          /* icp.hasConverged()                                       */
    int32_t state;              /* rsreg_convergence_state                                  */
    int32_t iterations;         /* nr_iterations_                                           */
    int32_t reserved0;
    uint64_t n_correspondences; /* pairs accepted in the last iteration                     */
    double mse;                 /* mean squared distance of those pairs (last iteration)    */
    double sums_last[RSREG_NUM_SUMS]; /* the 17 sums of the last iteration (point-to-plane: [0] and [16] -- the
                                         plane sums [0] and [1] -- the rest 0; all 32: rsreg_icp_plane_sums_last) */
    /* device-time breakdown of this call (ms, HIP events on the ctx stream); 0 if profiling off */
    double ms_total;
    double ms_nn;               /* dominant kernel: NN search (or the fused kernel)         */
    double ms_reduce;           /* staged: the sums kernels; fused: all time between consecutive search
                                   kernels (final reduce + host round trip or device solve)            */
    double ms_transform;
    int32_t n_nn_launches;
    int32_t n_scheduled_launches; /* ... of them launched from the tile schedule (fused dense kernel: DESIGN.md §4)       */
    double ms_allreduce;        /* N > 1 ranks: the all-reduce of the 17 sums, all iterations (0.3; 0 with one rank)   */
} rsreg_icp_result;

typedef struct rsreg_ndt_result {
    float transform[16];
    int32_t converged;
    int32_t iterations;
    double trans_probability;   /* ndt.getTransformationProbability()                       */
    double score;
    int32_t n_voxels;           /* valid target voxels (>= 6 points, invertible covariance)  */
    int32_t n_derivative_passes;
    double ms_total;
    double ms_derivatives;
} rsreg_ndt_result;

/* ---- library / device ------------------------------------------------------------ */
int rsreg_version(void);                        /* major*1000 + minor */
const char *rsreg_status_string(int status);
const char *rsreg_last_error(const rsreg_ctx *ctx); /* detail of the last failure on ctx   */
int rsreg_device_count(int *count);

/* stream: a hipStream_t to run on (e.g. torch's current stream), or NULL for a new one. */
int rsreg_ctx_create(int device_id, void *stream, rsreg_ctx **out);
int rsreg_ctx_destroy(rsreg_ctx *ctx);
int rsreg_ctx_synchronize(rsreg_ctx *ctx);
/* What a frame loop is about to need, requested ahead of the need (engine extra; the schemes call it when registration() starts:
 * types.hpp:19, main.cpp:85 -- the first registration() of a process otherwise creates these one by one on its critical
 * path): the context's upload / source / download streams and, with RSREG_PREPARE_SIDE_STREAMS, the four side streams
 * (hardware queues: ~12 ms each for a process's first four), the pinned staging buffers of the upload and download workers
 * for frames of `frame_bytes` (0: none), and one device buffer of `model_bytes` for a cloud that will grow to that size
 * (0: none; the merged model of IncrementalICP then grows without re-allocation).  Returns at once: a thread of the context
 * makes them while the caller goes on; every entry point that needs one of them waits for that thread first.  Call it while no
 * upload or download of the context is in flight (between registrations).  Optional: without it everything is created at first
 * use, as before. */
#define RSREG_PREPARE_SIDE_STREAMS 1u
int rsreg_ctx_prepare(rsreg_ctx *ctx, size_t frame_bytes, size_t model_bytes, unsigned flags);
int rsreg_ctx_set_profiling(rsreg_ctx *ctx, int enabled);

void rsreg_icp_params_default(rsreg_icp_params *p);
void rsreg_icp_params_reference(rsreg_icp_params *p);
void rsreg_ndt_params_default(rsreg_ndt_params *p);
void rsreg_ndt_params_reference(rsreg_ndt_params *p);

/* ---- ICP: pcl::IterativeClosestPoint<PointXYZRGB,PointXYZRGB> ------------------------ */

/* icp.setInputTarget(cloud) + the search-structure build PCL does in initCompute()
 * (incremental_icp.hpp:58, icp_edge...hpp:79,109, ndt_edge...hpp:97).  Builds the
 * uniform-grid index over the finite target points.  The grid cell size is derived from
 * max_correspondence_distance, so that must be known here.
 * The build is QUEUED on the context's stream and may not be finished when the call returns (its two counts are
 * taken over at the next call that waits for the stream): a host buffer has been read by then (a second
 * rsreg_icp_set_target first waits for the queued build that still reads the staged records); a DEVICE buffer
 * (d_points) must stay alive and unchanged until the next synchronising call on the context -- rsreg_icp_align /
 * rsreg_icp_begin, rsreg_icp_grid_info or rsreg_ctx_synchronize -- has returned.
 * RANGE.  The grid is decided by csrc/icp_grid_plan.hpp from the box of the finite records, their number and the gate; its
 * constants are metres (a cell cap of 14 .. 42 mm, at most 60 000 cells along the longest axis, at least 1e-6 m a cell), so a
 * cloud at another scale gets another grid.  A target is SERVED when that grid's cell is at most 2^60 m (1.15e18) and the box
 * is no wider than a finite float along any axis; every other target -- a cloud of extent 6.9e22 m or more, a bounded gate of
 * 8.9e18 m or more, records at +-3e38 -- is taken (its records and box serve rsreg_icp_fitness_score, which searches an index
 * of its own over the whole float range) but every correspondence search over it -- rsreg_icp_search, rsreg_icp_align* -- is
 * REFUSED with RSREG_ERR_INVALID_ARG: on such a grid cell * cell is not a normal float and the searches' bounds would skip cells
 * that hold the answer.  Nothing is refused for being small: a cloud of denormal coordinates lies in one cell and is searched
 * point by point.
 * COST.  A search looks at nothing farther than the gate.  With an UNBOUNDED gate (PCL's default, sqrt(DBL_MAX)) or one wider
 * than the cloud, a query with no target point near it walks the grid outwards until the grid is exhausted: up to
 * (longest axis in cells / 2)^3 bricks of the brick hash, or (2 * longest axis)^2 rows of the dense table.  For a cloud of a few
 * metres that is a few thousand steps; for a cloud wider than about 2.5 km the cell is extent / 60 000 whatever the number of
 * points, and one such query costs up to 10^13 steps -- in practice the call does not return.  Give a cloud of that extent a
 * gate below a quarter of its extent: the cell then follows the gate, and a query costs a few thousand steps at most
 * (tests/icp_grid_layout.py: cost_bound, the model; tests/icp_scale_cases.py: OVER_CAP, the cases left out for it). */
int rsreg_icp_set_target(rsreg_ctx *ctx, const void *points, size_t n, size_t stride,
                         int is_dense, double max_correspondence_distance);
int rsreg_icp_set_target_device(rsreg_ctx *ctx, const void *d_points, size_t n, size_t stride,
                                int is_dense, double max_correspondence_distance);

/* icp.setInputSource(cloud) (incremental_icp.hpp:57, icp_edge...hpp:78,108).  The source is put into the
 * engine's order on a stream of its own and joined when the alignment begins: called BEFORE rsreg_icp_set_target
 * (the reference's order) it runs beside the target's index build.  A host buffer is consumed before the call
 * returns (packed into pinned memory; its way over the PCIe link goes on while the caller packs the target); a device
 * buffer must stay alive and unchanged until rsreg_icp_begin / rsreg_icp_align has returned. */
int rsreg_icp_set_source(rsreg_ctx *ctx, const void *points, size_t n, size_t stride, int is_dense);
int rsreg_icp_set_source_device(rsreg_ctx *ctx, const void *d_points, size_t n, size_t stride,
                                int is_dense);

/* icp.align(out) / icp.align(out, guess) + hasConverged() + getFinalTransformation()
 * (incremental_icp.hpp:59-63, icp_edge...hpp:95,104,111-117, ndt_edge...hpp:99-105).
 * guess: 16 floats column-major, NULL = identity.  aligned_out (nullable, host): receives
 * n_source records of `out_stride` bytes: the input records with xyz <- final * xyz
 * (only xyz and, if out_stride >= 16, data[3] = 1 are written; copy colour yourself). */
int rsreg_icp_align(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params,
                    rsreg_icp_result *result, void *aligned_out, size_t out_stride);
/* The same with PCL's `output = input` done on the way (incremental_icp.hpp:59 `icp.align(*aligned)`: PCL copies the input cloud
 * into the output and then rewrites xyz): aligned_out receives n_source WHOLE records of `stride` bytes -- the records at
 * `source_records` (the host cloud the source was set from, or any records of that layout; may be aligned_out itself) with
 * xyz <- final * xyz and, if stride >= 16, data[3] = 1.  The copy is made by the host threads that write the aligned positions
 * anyway, while those are still on the PCIe link: an adaptor no longer copies 32 bytes a point itself before the call
 * (2.5 -> 1.9 ms per 10^6-point pair). */
int rsreg_icp_align_records(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params,
                            rsreg_icp_result *result, const void *source_records, void *aligned_out, size_t stride);

/* Step-wise form of the same loop (parity tests, N-GPU sharding by source blocks):
 *   begin -> { search -> sums -> [all-reduce the 17 sums] -> update } ... -> end     */
int rsreg_icp_begin(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params);
/* CorrespondenceEstimation::determineCorrespondences: nearest target per current source
 * point.  Outputs (host, each nullable, n_source entries): index into the ORIGINAL target
 * array (-1: no target within the gate / non-finite source point), squared distance.
 * The contract is a float32 brute force: d2 = (dx * dx + dy * dy) + dz * dz, every operation rounded once (a difference that
 * overflows gives +inf, a square that underflows a denormal or 0); the lowest target index among the smallest d2 (+inf ties
 * with +inf); a pair is rejected iff (double)d2 > gate * gate.  It holds, index for index and d2 bit for bit, over every served
 * target (rsreg_icp_set_target: RANGE) for every finite query, wherever it lies -- tests/test_icp_scale_gpu.py: clouds from 2^-140
 * to 2^66, offsets up to 2^23 m, queries 2^5 .. 2^100 m outside the box, a gate of +inf under which pairs at d2 = +inf are accepted,
 * on both kinds of index.  A query more than 1 024 cells outside the target's box (its position in cell units then carries a
 * rounding the bounds' margin is not argued for) is searched without bounds: nothing when the gate cannot reach the box from
 * there, else every target point -- n points a query. */
int rsreg_icp_search(rsreg_ctx *ctx, int32_t *index_out, float *sqr_dist_out);
/* The 17 sums over the accepted correspondences of the last search (this rank's block). */
int rsreg_icp_sums(rsreg_ctx *ctx, double sums[RSREG_NUM_SUMS]);
/* TransformationEstimationSVD (Umeyama) from (possibly all-reduced) sums, transform the
 * source in place, compose final = T_inc * final, evaluate the convergence criteria.
 * t_inc_out (nullable): the incremental transform.  *done: 1 when the loop must stop. */
int rsreg_icp_update(rsreg_ctx *ctx, const double sums[RSREG_NUM_SUMS], float *t_inc_out,
                     int *done);
int rsreg_icp_end(rsreg_ctx *ctx, rsreg_icp_result *result, void *aligned_out, size_t out_stride);

/* Registration::getFitnessScore(max_range) (PCL 1.9 registration.hpp) after an alignment of this context: the source as it was
 * handed in -- every record, exact copies once per record, in the caller's order -- moved by the final 4x4 of that alignment
 * (guess included) with rsreg_transform_cloud's arithmetic; for each finite point the squared float distance d2 to its nearest
 * finite target point, at ANY distance (not limited by the correspondence gate the target's index was built for); the mean of
 * the d2 with d2 <= max_range.  *score = that mean, DBL_MAX when no point is in range (not an error); *n_within (nullable) =
 * how many records were.
 * PCL's quirk, kept: max_range is compared with the SQUARED distance (`if (nn_dists[0] <= max_range)`), not the distance;
 * the default of getFitnessScore() is DBL_MAX (everything counts).  Non-finite source points are neither counted nor summed;
 * the correspondence filters (reciprocal, trimmed) do not apply, as PCL's fitness score ignores rejectors.
 * Valid after a completed alignment (rsreg_icp_align, _align_records, _align_cloud, rsreg_icp_end) until the next
 * set_source / set_target, RSREG_ERR_STATE before.  Neither call changes the alignment's index or any later result: the
 * search runs over an index of its own, built at the first call after a target change.
 * With a communicator of more than one rank, rsreg_icp_fitness_score all-reduces the two numbers through it (each rank holds a
 * block of the source); rsreg_icp_fitness_sums never does: sums[0] = this rank's count, sums[1] = its sum of d2 (f64), for
 * callers that reduce across ranks themselves. */
int rsreg_icp_fitness_score(rsreg_ctx *ctx, double max_range, double *score, uint64_t *n_within);
int rsreg_icp_fitness_sums(rsreg_ctx *ctx, double max_range, double sums[2]);

/* Host-only pieces of the iteration, exposed for tests and for callers that run the
 * all-reduce themselves. */
int rsreg_umeyama_from_sums(const double sums[RSREG_NUM_SUMS], float t_out[16]);

/* ---- point-to-plane ICP: pcl::IterativeClosestPointWithNormals (params->estimation = RSREG_ESTIMATION_POINT_TO_PLANE_LLS) ---- */
/* The target's normals, one per target RECORD in the caller's order: three floats at `normals + i * stride` (pcl::Normal
 * records: stride 32; PointXYZRGBNormal records: stride 48 with the pointer at normal_x).  Call it after
 * rsreg_icp_set_target*; n must be that target's record count (RSREG_ERR_INVALID_ARG otherwise, RSREG_ERR_NO_TARGET without a
 * target); any later rsreg_icp_set_target* drops the normals.  The host buffer has been read when the call returns.
 * _cloud: a device cloud of the context, e.g. what rsreg_cloud_normals wrote (read on the context's stream: keep it alive
 * and unchanged until the next synchronising call has returned).  An alignment in plane mode without normals:
 * RSREG_ERR_STATE from rsreg_icp_begin.  rsreg_icp_align, _align_records, _align_cloud, rsreg_icp_end and the fitness score
 * work as for point-to-point; source normals, where the records carry any, are copied, not rotated. */
int rsreg_icp_set_target_normals(rsreg_ctx *ctx, const void *normals, size_t n, size_t stride);
int rsreg_icp_set_target_normals_cloud(rsreg_ctx *ctx, const rsreg_cloud *normals);
/* Step-wise form: begin -> { search -> plane_sums -> update_plane } ... -> end.  The 32 sums (RSREG_NUM_PLANE_SUMS above)
 * over the accepted correspondences of the last search; the solve, compose and criteria of rsreg_icp_update from them
 * (ncorr = [0], mse = [1] / [0]; ncorr < 3: RSREG_CONV_NO_CORRESPONDENCES).  In plane mode rsreg_icp_sums and
 * rsreg_icp_update return RSREG_ERR_STATE, and these two do in point-to-point mode. */
int rsreg_icp_plane_sums(rsreg_ctx *ctx, double sums[RSREG_NUM_PLANE_SUMS]);
int rsreg_icp_update_plane(rsreg_ctx *ctx, const double sums[RSREG_NUM_PLANE_SUMS], float *t_inc_out, int *done);
/* The 32 sums of the last iteration of the last plane alignment (all 0 after a point-to-point one). */
int rsreg_icp_plane_sums_last(rsreg_ctx *ctx, double sums[RSREG_NUM_PLANE_SUMS]);
/* The solve alone (host only, no ctx): t_out = the increment, column-major; *rank_out (nullable) = eigen-directions used. */
int rsreg_plane_solve_from_sums(const double sums[RSREG_NUM_PLANE_SUMS], float t_out[16], int *rank_out);

/* ---- correspondence rejectors: pcl::Registration::addCorrespondenceRejector ------------------------------------------------
 * An ordered chain of rejectors on the context, applied in every ICP iteration between determineCorrespondences and the
 * transformation estimate, for point-to-point and point-to-plane estimation alike.  The rules are RECALLED FROM PCL 1.9.1
 * (registration/correspondence_rejection_*.{h,cpp}, icp.hpp) and CANNOT BE PINNED WITHOUT PCL; the deviations are stated.
 *
 * WHERE THE CHAIN SITS.  A pair is IN PLAY when its source record is finite, has a target within the gate, has passed the
 * reciprocal test if rsreg_icp_params.use_reciprocal_correspondences is on and the trim if trim_overlap_ratio is set: those two
 * run first, as without a chain.  The chain then runs in the order given, each rejector over what the one before left, as PCL's
 * loop feeds each rejector the previous one's getCorrespondences.  It works on ORIGINAL source records in the caller's order on
 * both source paths (up to 65 536 records searched as they come; larger sources, or RSREG_SORT_SMALL=1, merged into weighted
 * distinct points): copies of a point are separate pairs, every tie goes to the lowest source index, and a rejector may keep any
 * subset of a point's copies (exact copies may carry different normals).  A non-empty chain makes the iteration run as
 * RSREG_PIPELINE_STAGED whatever pipeline_mode asks for, like the two filters, and makes a target that was set without an index
 * build it.  A context whose communicator has more than one rank refuses a non-empty chain (RSREG_ERR_INVALID_ARG from
 * rsreg_icp_begin).  The chain stays on the context until replaced; an alignment uses the chain rsreg_icp_begin found.
 * rsreg_icp_fitness_score and the rsreg_gicp_* entry points ignore it (PCL's fitness score and PCL's GICP loop consult no
 * rejector).  Behind the chain, fewer than 3 pairs ([0] of the 17 or 32 sums) end the alignment with
 * RSREG_CONV_NO_CORRESPONDENCES, as without one.  An empty chain -- the default -- changes nothing at all.
 * The whole chain is queued on the context's stream and adds no host wait to an iteration; it uses integer atomics only, so
 * the same chain on the same inputs keeps the same pairs and gives the same sums on any context, at any launch.
 *
 * RSREG_REJECTOR_MEDIAN_DISTANCE (CorrespondenceRejectorMedianDistance, value = setMedianFactor, PCL default 1.0).  m = the pairs
 * in play; m == 0: nothing happens.  The median is the float d2 at 0-based rank floor(m / 2) of the in-play d2 in ascending
 * order: the upper median, PCL's nth_element(begin + size / 2).  A pair stays iff (double)d2 <= (double)median * factor,
 * evaluated as written in IEEE double: a pair at the bound stays, a NaN product (0 * inf) drops every pair.  factor must not be
 * NaN or negative.  The d2 is the one the search returned.  DEVIATION: PCL's ICP hands the rejector a data container through
 * which it recomputes the distance from the clouds -- the same quantity in another rounding.
 * RSREG_REJECTOR_ONE_TO_ONE (CorrespondenceRejectorOneToOne).  Of the pairs in play that share a target record the one with the
 * smallest (d2, source index) stays.  DEVIATION: PCL's std::sort leaves the order of equal distances open; the lowest source
 * index is this library's rule.
 * RSREG_REJECTOR_SURFACE_NORMAL (CorrespondenceRejectorSurfaceNormal, DataContainer::getCorrespondenceScoreFromNormals, value =
 * setThreshold, a cosine, PCL default 1.0).  A pair stays iff (double)((sx*tx + sy*ty) + sz*tz) > threshold: float arithmetic,
 * every operation rounded once, no contraction; the comparison is strict; a NaN score drops the pair.  t = the matched target
 * RECORD's normal (rsreg_icp_set_target_normals*).  s = the source record's CURRENT normal: the one handed in
 * (rsreg_icp_set_source_normals*), turned at rsreg_icp_begin by the guess's 3 x 3 block -- (r0*x + r1*y) + r2*z per row, the
 * arithmetic of rsreg_transform_cloud without the translation; an identity guess copies it -- and after every update turned in
 * place by the increment's 3 x 3 block, as the points are moved (PCL transforms its working cloud's normals with each increment
 * too).  A chain with this kind and either set of normals missing: RSREG_ERR_STATE from rsreg_icp_begin.  A new rsreg_icp_begin
 * on the same source starts again from the normals as handed in.
 * RSREG_REJECTOR_TRIMMED (CorrespondenceRejectorTrimmed, value = setOverlapRatio, 0 < r < 1, anything else:
 * RSREG_ERR_INVALID_ARG).  The rule of trim_overlap_ratio at that place of the chain, over the pairs in play there: the same
 * kernels, the first floor((float)r * (float)count) pairs in (d2, source index) order stay.  rsreg_icp_params.trim_overlap_ratio
 * keeps its place in front of the chain.
 *
 * rsreg_icp_set_rejectors: n = 0 clears the chain; at most 8 entries; an unknown kind, a bad value or n > 8:
 * RSREG_ERR_INVALID_ARG, and the chain set before stays.
 * rsreg_icp_rejector_stats: valid after a rsreg_icp_search (or an alignment) with a chain, until the next search;
 * RSREG_ERR_STATE otherwise.  One record per chain entry, as many as `capacity` holds; n_in / n_out = the pairs in front of and
 * behind the entry, counted in original records; median_distance = the median d2 of a MEDIAN_DISTANCE entry
 * (getMedianDistance()), 0 when m == 0 and for the other kinds.  *n_out (nullable) = the chain's length, which may exceed
 * `capacity`.  This call waits for the stream; nothing else of the chain does.
 * rsreg_icp_search's index_out / sqr_dist_out report -1 for every record the chain dropped, as for the two filters.
 * rsreg_icp_set_source_normals*: one normal per source RECORD in the caller's order, layout and lifetime as
 * rsreg_icp_set_target_normals*.  Call it after rsreg_icp_set_source*; n must be that source's record count
 * (RSREG_ERR_INVALID_ARG otherwise, RSREG_ERR_NO_SOURCE without a source); any later rsreg_icp_set_source* drops them.
 * NOT BUILT: CorrespondenceRejectorVarTrimmed, ...Distance (max_correspondence_distance is it), ...Features, ...Poly inside ICP,
 * rejectors over a stand-alone correspondence list, and the chain across ranks. */
typedef enum rsreg_rejector_kind {
    RSREG_REJECTOR_MEDIAN_DISTANCE = 1,   /* value = factor,    PCL default 1.0 */
    RSREG_REJECTOR_ONE_TO_ONE      = 2,   /* value unused                        */
    RSREG_REJECTOR_SURFACE_NORMAL  = 3,   /* value = threshold (a cosine), PCL default 1.0 */
    RSREG_REJECTOR_TRIMMED         = 4    /* value = overlap ratio, 0 < r < 1    */
} rsreg_rejector_kind;
typedef struct rsreg_rejector { int32_t kind; int32_t reserved0; double value; } rsreg_rejector;
typedef struct rsreg_rejector_stat { uint64_t n_in, n_out; double median_distance; double reserved0; } rsreg_rejector_stat;
#define RSREG_MAX_REJECTORS 8

int rsreg_icp_set_rejectors(rsreg_ctx *ctx, const rsreg_rejector *chain, int32_t n);      /* n = 0 clears; at most 8 */
int rsreg_icp_rejector_stats(rsreg_ctx *ctx, rsreg_rejector_stat *stats, int32_t capacity, int32_t *n_out);
int rsreg_icp_set_source_normals(rsreg_ctx *ctx, const void *normals, size_t n, size_t stride);
int rsreg_icp_set_source_normals_cloud(rsreg_ctx *ctx, const rsreg_cloud *normals);

/* ---- GICP: pcl::GeneralizedIterativeClosestPoint (plane-to-plane ICP, Segal et al.) ------------------------------------------
 * A sibling of point-to-plane ICP with entry points of its own (rsreg_icp_params.estimation has no value for it): the context's
 * ICP source, target, index and staged search are shared -- the clouds come in through rsreg_icp_set_source* / rsreg_icp_set_target*
 * -- and every correspondence is weighted by the surface covariance of both clouds.  PCL 1.9.1 (registration/gicp.h, impl/gicp.hpp)
 * is recalled, not read; what is kept from it: the objective, the correspondences, the Mahalanobis matrices, the defaults and the
 * outer stopping rule.  DEVIATIONS, stated where they apply: (1) the covariance is rebuilt as I - (1 - epsilon) n n^T, not through
 * an SVD; (2) every sum is f64 in a fixed order; (3) the inner minimiser is Gauss-Newton with step halving, not PCL's BFGS.
 *
 * COVARIANCES (rsreg_cloud_gicp_covariances; PCL: computeCovariances, k = setCorrespondenceRandomness, default 20, epsilon =
 * gicp_epsilon_, default 0.001).  For every finite record q of `in`: its k nearest neighbours t_1 .. t_k as rsreg_cloud_knn returns
 * them, the record itself and exact copies included, 4 <= k <= 64 (RSREG_ERR_INVALID_ARG otherwise, and when fewer than k records
 * are finite); the moments of d_i = t_i - q in f64, c = (sum d d^T) / k - (sum d / k)(sum d / k)^T -- the sums, their order and the
 * covariance are those of rsreg_cloud_normals; n = the unit eigenvector of c's smallest eigenvalue by the same Jacobi, (0, 0, 1) when
 * trace(c) == 0 (all neighbours coincide); then, every operation rounded once, no contraction, s = 1 - epsilon:
 *     C'_ab = delta_ab - s * (n_a * n_b)                 (a diagonal entry: 1 - s * (n_a * n_a); another: 0 - s * (n_a * n_b))
 * PCL replaces the singular values of c by (1, 1, epsilon) and rebuilds U diag(1, 1, epsilon) U^T; with U orthonormal that is the
 * matrix above.  DEVIATION (1): the rounding order differs from PCL's SVD rebuild (and PCL's moments are sums about the origin in
 * its own neighbour order); where the two smallest eigenvalues of c coincide, n is any unit vector of their plane, here as there.
 * out: one 48-byte record per input record, six doubles (xx, xy, xz, yy, yz, zz), width and height of the input; a non-finite input
 * record gets six quiet NaNs and makes the cloud not dense, otherwise is_dense is the input's.  The result depends on the cloud
 * alone, not on the launch or the context.
 *
 * PARAMETERS (rsreg_gicp_params_default = PCL 1.9.1 gicp.h, recalled: 200, 20, 5.0, 5e-4, 2e-3, 20, 1e-3).  k_correspondences and
 * gicp_epsilon are what the C++ and Python classes hand to rsreg_cloud_gicp_covariances when the caller gave no covariances; the
 * alignment itself reads the covariances that were set.
 *
 * SETTING THE COVARIANCES.  One 48-byte-or-wider record of six doubles per source (target) RECORD, in the caller's order, n = the
 * record count of the cloud set by rsreg_icp_set_source* (rsreg_icp_set_target*): RSREG_ERR_INVALID_ARG otherwise, RSREG_ERR_NO_SOURCE
 * / RSREG_ERR_NO_TARGET without the cloud; stride >= 48 (a device cloud: a multiple of 8).  The next rsreg_icp_set_source*
 * (rsreg_icp_set_target*) drops them.  The host buffer has been read when the call returns; a device cloud is read on the context's
 * stream.  Exact copies of a source point have the same neighbours and so the same covariance: the engine's merged copies use the
 * first copy's record and the pair weight W below.
 *
 * ONE OUTER ITERATION (T = the current transform, float 4 x 4, the guess at first; R = its rotation block, float -> double):
 * 1. Search: the source under T (from the records, not incrementally), rsreg_icp_search's exact nearest neighbour and gate
 *    (a pair is rejected iff (double)d2 > max_correspondence_distance^2).  p = the moved source point (float), q = its target.
 * 2. Per kept pair (source record i, target record j), in f64, every operation rounded once:
 *      B = R C_s[i]:  B_rc = (R_r0 C_0c + R_r1 C_1c) + R_r2 C_2c        D = B R^T:  D_rc = (B_r0 R_c0 + B_r1 R_c1) + B_r2 R_c2   (c >= r)
 *      A = C_t[j] + D      adjugate: a00 = A11 A22 - A12 A12   a01 = A02 A12 - A01 A22   a02 = A01 A12 - A02 A11
 *                                    a11 = A00 A22 - A02 A02   a12 = A01 A02 - A00 A12   a22 = A00 A11 - A01 A01
 *      det = (A00 a00 + A01 a01) + A02 a02      M_ab = a_ab * (1 / det)
 *    once per outer iteration, as PCL computes mahalanobis_.  Both summands have eigenvalues >= epsilon, so finite covariances give
 *    a finite M.  A pair with a non-finite entry in C_s[i] or C_t[j], or in M, is SKIPPED: it adds to sums [0] and [1] only (PCL's
 *    rule, the one plane mode follows for NaN normals).
 * 3. Inner minimisation of sum W e^T M e over an increment X (double 4 x 4, I at first) applied on the left of the moved points:
 *      p' = X p:  p'_r = ((X_r0 p.x + X_r1 p.y) + X_r2 p.z) + X_r3      e = q - p'      J = [-[p']x | I3]  (small angles, as plane mode)
 *      g = M e:  g_r = (M_r0 e_0 + M_r1 e_1) + M_r2 e_2      G = [p']x M:  G_0c = p'y M_2c - p'z M_1c   G_1c = p'z M_0c - p'x M_2c
 *                                                                           G_2c = p'x M_1c - p'y M_0c
 *    The 32 sums at X (RSREG_NUM_GICP_SUMS, all f64; W = how many source records the pair stands for):
 *      [0] sum W over the gated pairs      [1] sum W * (double)d2 of the search -- bit-equal to rsreg_icp_sums [0] and [16]
 *      [2] sum W over the pairs in the system      [3] sum W * ((e_0 g_0 + e_1 g_1) + e_2 g_2), the cost
 *      [4..24] H = sum W J^T M J, upper triangle row-major (00 01 .. 05 11 .. 55):
 *              rows 0-2 x cols 0-2: H_r0 = G_r2 p'y - G_r1 p'z   H_r1 = G_r0 p'z - G_r2 p'x   H_r2 = G_r1 p'x - G_r0 p'y
 *              rows 0-2 x cols 3-5: G      rows 3-5 x cols 3-5: M
 *      [25..30] b = sum W J^T M e = (p'y g_2 - p'z g_1,  p'z g_0 - p'x g_2,  p'x g_1 - p'y g_0,  g_0, g_1, g_2)      [31] 0
 *    in the fixed addition order of the plane sums (per tile by halving over lanes, then the tiles): the same 32 doubles on any
 *    context, at any launch.  x = pinv(H) b by rsreg_plane_solve_from_sums' rule (same eigenvalue cut over [2]) is the Gauss-Newton
 *    step, and Delta(x) = PCL's constructTransformationMatrix(x), kept in double.
 *    Step control, decided by the sums alone:  S = sums(I);  repeat { x = solve(S), stop if its rank is 0;  c = 1;
 *      repeat { X' = Delta(c x) X  (entries ((a0 b0 + a1 b1) + a2 b2) + a3 b3);  S' = sums(X');  accept (X, S <- X', S') if S'[3] <= S[3],
 *      else c <- c / 2 };  stop if every |c x_0..2| <= rotation_epsilon and every |c x_3..5| <= transformation_epsilon }.
 *    Every evaluation after the first counts against max_inner_iterations; the loop ends where they are used up (a step not yet
 *    accepted is dropped).
 *    DEVIATION (3): PCL minimises the same objective over (t, Euler angles) with its own BFGS port and line search.
 * 4. T_new = float(X T), entries ((X_r0 T_0c + X_r1 T_1c) + X_r2 T_2c) + X_r3 T_3c in double.  PCL's test, recalled: delta = the
 *    largest |T(k,l) - T_new(k,l)| over the 3 x 4 block times 1 / rotation_epsilon (l < 3) or 1 / transformation_epsilon (l = 3)
 *    (an entry that did not change counts 0 whatever the epsilon); the loop stops when delta < 1 (RSREG_CONV_TRANSFORM) or the
 *    iteration count reaches max_iterations (RSREG_CONV_ITERATIONS); converged is 1 in both cases, as PCL sets it.  Fewer than 4
 *    pairs in [0]: RSREG_CONV_NO_CORRESPONDENCES, converged 0, the transform as it was.
 *
 * CALLS.  rsreg_gicp_align[_cloud] runs the loop (aligned_out as rsreg_icp_align[_cloud]).  Step-wise, for tests and callers with a
 * loop of their own:  begin -> { search -> sums(X) ... -> update(X) } -> end.  rsreg_gicp_search: step 1 and 2 (outputs as
 * rsreg_icp_search); rsreg_gicp_sums: the 32 sums at X (column-major 4 x 4, NULL = I) of the last search; rsreg_gicp_step_from_sums
 * (host only, no ctx): x_out = scale * pinv(H) b, delta_out = Delta(x_out) column-major (identity when the rank is 0);
 * rsreg_gicp_update: step 4 with the caller's X and the sums at it (n_correspondences, mse = [1] / [0]; inner_evaluations adds to
 * the result's count), *done = 1 when the loop must stop.  Alignments without both covariance sets: RSREG_ERR_STATE from
 * rsreg_gicp_begin; a communicator of more than one rank: RSREG_ERR_INVALID_ARG (nothing is all-reduced).  rsreg_icp_fitness_score
 * works after a GICP alignment as after any other. */
#define RSREG_NUM_GICP_SUMS 32

typedef struct rsreg_gicp_params {
    int32_t max_iterations;             /* setMaximumIterations, 200                                  */
    int32_t max_inner_iterations;       /* setMaximumOptimizerIterations, 20                          */
    int32_t k_correspondences;          /* setCorrespondenceRandomness, 20                            */
    int32_t reserved0;
    double max_correspondence_distance; /* setMaxCorrespondenceDistance, 5.0                          */
    double transformation_epsilon;      /* setTransformationEpsilon, 5e-4                             */
    double rotation_epsilon;            /* setRotationEpsilon, 2e-3                                   */
    double gicp_epsilon;                /* gicp_epsilon_, 1e-3                                        */
} rsreg_gicp_params;

typedef struct rsreg_gicp_result {
    float transform[16];        /* final_transformation_, column-major                               */
    int32_t converged;
    int32_t state;              /* rsreg_convergence_state: ITERATIONS, TRANSFORM or NO_CORRESPONDENCES */
    int32_t iterations;         /* outer iterations                                                  */
    int32_t inner_evaluations;  /* evaluations of the 32 sums after the first of every outer iteration, all iterations */
    uint64_t n_correspondences; /* [0] of the last iteration                                         */
    double mse;                 /* [1] / [0] of the last iteration                                   */
    double sums_last[RSREG_NUM_GICP_SUMS]; /* the 32 sums at the accepted X of the last iteration  */
    double ms_total;            /* device-time breakdown as rsreg_icp_result (0 if profiling off)    */
    double ms_nn;
    double ms_reduce;           /* the Mahalanobis and sums kernels                                  */
    double ms_transform;
    int32_t n_nn_launches;
    int32_t rank_last;          /* eigen-directions the last solve used                              */
} rsreg_gicp_result;

void rsreg_gicp_params_default(rsreg_gicp_params *p);
int rsreg_cloud_gicp_covariances(rsreg_ctx *ctx, const rsreg_cloud *in, int k, double epsilon, rsreg_cloud *out);
int rsreg_gicp_set_source_covariances(rsreg_ctx *ctx, const void *cov, size_t n, size_t stride);
int rsreg_gicp_set_target_covariances(rsreg_ctx *ctx, const void *cov, size_t n, size_t stride);
int rsreg_gicp_set_source_covariances_cloud(rsreg_ctx *ctx, const rsreg_cloud *cov);
int rsreg_gicp_set_target_covariances_cloud(rsreg_ctx *ctx, const rsreg_cloud *cov);
int rsreg_gicp_begin(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params);
int rsreg_gicp_search(rsreg_ctx *ctx, int32_t *index_out, float *sqr_dist_out);
int rsreg_gicp_sums(rsreg_ctx *ctx, const double X[16], double sums[RSREG_NUM_GICP_SUMS]);
int rsreg_gicp_step_from_sums(const double sums[RSREG_NUM_GICP_SUMS], double scale, double x_out[6], double delta_out[16], int *rank_out);
int rsreg_gicp_update(rsreg_ctx *ctx, const double X[16], const double sums[RSREG_NUM_GICP_SUMS], int inner_evaluations, int *done);
int rsreg_gicp_end(rsreg_ctx *ctx, rsreg_gicp_result *result, void *aligned_out, size_t out_stride);
int rsreg_gicp_align(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, rsreg_gicp_result *result,
                     void *aligned_out, size_t out_stride);
int rsreg_gicp_align_cloud(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, rsreg_gicp_result *result,
                           rsreg_cloud *aligned_out);

/* ---- GICP6D: pcl::GeneralizedIterativeClosestPoint6D (registration/gicp6d.h) -------------------------------------------------
 * GICP whose correspondences are nearest neighbours in (x, y, z, w L', w a', w b'): the colour of a PointXYZRGB record decides
 * between candidates that geometry cannot tell apart (a wall, a floor, a table top leave the in-plane part of a pose free under
 * plane-to-plane ICP).  The covariances, the Mahalanobis pass, the 32 sums, the step control and the stopping rule are GICP's,
 * above, untouched.  RECALLED from PCL 1.9.1 (gicp6d.h / gicp6d.cpp; no test here holds them against PCL): the two-table shape of RGB2Lab and
 * its coefficients, the normalisation L / 100, a / 120, b / 120, the default weight 0.032, the rescaling of the colour
 * coordinates before the tree sees the vector, FLANN's L2_Simple over the six coordinates.  THIS LIBRARY'S: everything marked
 * "deviation" below, the clamps, the gate and tie rules, what a non-finite coordinate does, and the index.
 *
 * COLOUR (rsreg_lab_tables, rsreg_rgb_to_lab, rsreg_cloud_lab).  Every operation is a float operation rounded once, nothing fused:
 *    r, g, b = bits 16-23, 8-15, 0-7 of the uint32 at byte 16 of the record (as rsreg_extract_edge_features reads it); a cloud of
 *      stride < 20: RSREG_ERR_INVALID_ARG.
 *    S[i], i = 0 .. 255:  f = i / 255.0;   f > 0.04045 ? pow((f + 0.055) / 1.055, 2.4) : f / 12.92     in double, rounded to float
 *    F[i], i = 0 .. 3999: f = i / 4000.0;  f > 0.008856 ? cbrt(f) : 7.787 * f + 16.0 / 116.0           in double, rounded to float
 *      (deviation: PCL fills both tables with powf in float)
 *    x = (S[r] * 0.412453f + S[g] * 0.357580f) + S[b] * 0.180423f
 *    y = (S[r] * 0.212671f + S[g] * 0.715160f) + S[b] * 0.072169f
 *    z = (S[r] * 0.019334f + S[g] * 0.119193f) + S[b] * 0.950227f
 *    vx = x / 0.95047f, vy = y, vz = z / 1.08883f;  table index (int)(v * 4000.0f) clamped to 0 .. 3999
 *      (deviation: PCL does not clamp, and white indexes one past its table)
 *    L = 116.0f * F[vy] - 16.0f, capped at 100;  a = 500.0f * (F[vx] - F[vy]),  b = 200.0f * (F[vy] - F[vz]), both clamped to +-120
 *    out = L / 100.0f, a / 120.0f, b / 120.0f  (normalised as PCL's 6-D point is).  The colour does not depend on x, y, z: a record
 *      with non-finite coordinates still gets its colour.
 * rsreg_lab_tables (host only, no context) returns S and F as the library uses them; rsreg_rgb_to_lab (host only) is the formula
 * over n packed words, lab_out n x 3 floats; rsreg_cloud_lab writes 16-byte records {L', a', b', 0.0f} with the width, height and
 * is_dense of `in` (out != in) -- the bytes of rsreg_rgb_to_lab.
 *
 * COLOURS OF AN ALIGNMENT (rsreg_gicp_set_source_lab / _target_lab and their _cloud forms): one record per cloud RECORD in the
 * caller's order whose first 12 bytes are L', a', b' (stride >= 12; a device cloud: a multiple of 4 -- what rsreg_cloud_lab wrote
 * fits), n = the cloud's record count (else RSREG_ERR_INVALID_ARG).  Lifetime and error codes as the covariance setters': set
 * after the cloud (RSREG_ERR_NO_SOURCE / _NO_TARGET before), dropped by the next rsreg_icp_set_source* / rsreg_icp_set_target*.
 *    The target's setter reads the target's RECORDS once more (their x, y, z): the alignment's index keeps one point per distinct
 *    position, and records that are copies in space but differ in colour are different candidates here.  A target from a host
 *    buffer has them in the context; a target set from device memory or a cloud handle must still lie there unchanged
 *    (RSREG_ERR_STATE if the handle's buffer has changed hands since).
 *    The source's setter takes a source that was merged into weighted distinct points (more than 65 536 records) apart again:
 *    EVERY SOURCE RECORD IS ITS OWN PAIR WITH ITS OWN COLOUR, W = 1 in the sums, and rsreg_icp_grid_info's n_source_distinct is the
 *    record count from then on, for every alignment of that source (same pairs per record; the sums add the same terms one by one).
 *
 * SEARCH (after rsreg_gicp6d_begin, rsreg_gicp_search runs it).  c = w * lab', w = (float)lab_weight, one float multiply per
 * coordinate, once per begin.  For a working point p (the source record under the current transform) and a target record t:
 *    d6 = ((((dx^2 + dy^2) + dz^2) + dL^2) + da^2) + db^2     differences, squares and sums each rounded once; the 3-D part is d2 of
 *      rsreg_icp_search, so w = 0 with finite colours gives that search's pairs
 *    the pair of p is the target record of smallest (d6, record index) among ALL finite target records -- exact, ties to the lowest
 *      index; a candidate whose d6 is NaN is skipped; a source record whose position or scaled colour is not finite gets no pair
 *    rejected (index -1) iff (double)d6 > max_correspondence_distance^2: rsreg_gicp_search's rule on the 6-D value.
 * index_out / sqr_dist_out, sums [1], mse and n_correspondences report d6.  The index is a grid over x, y, z of its own (every
 * finite record but those whose six coordinates equal, bit for bit, a record's of lower index: they can never win), built by the
 * first rsreg_gicp6d_begin after the target's colours were set; a bound on the 3-D
 * part bounds d6 (adding non-negative terms with round-to-nearest is monotone), so the walk is exact at any gate and for queries
 * anywhere.  rsreg_icp_fitness_score stays 3-D (PCL's getFitnessScore uses the plain tree).
 *
 * rsreg_gicp6d_begin = rsreg_gicp_begin + the colour checks: colours missing on either side RSREG_ERR_STATE; lab_weight NaN,
 * infinite or negative RSREG_ERR_INVALID_ARG.  rsreg_gicp_sums, _update and _end are unchanged; a later rsreg_gicp_begin searches in
 * three dimensions again.  rsreg_gicp6d_align[_cloud] runs rsreg_gicp_align's loop; PCL's default weight is 0.032. */
int rsreg_lab_tables(float srgb_out[256], float f_out[4000]);
int rsreg_rgb_to_lab(const uint32_t *rgba, size_t n, float *lab_out);
int rsreg_cloud_lab(rsreg_ctx *ctx, const rsreg_cloud *in, rsreg_cloud *out);
int rsreg_gicp_set_source_lab(rsreg_ctx *ctx, const void *lab, size_t n, size_t stride);
int rsreg_gicp_set_target_lab(rsreg_ctx *ctx, const void *lab, size_t n, size_t stride);
int rsreg_gicp_set_source_lab_cloud(rsreg_ctx *ctx, const rsreg_cloud *lab);
int rsreg_gicp_set_target_lab_cloud(rsreg_ctx *ctx, const rsreg_cloud *lab);
int rsreg_gicp6d_begin(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, double lab_weight);
int rsreg_gicp6d_align(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, double lab_weight,
                       rsreg_gicp_result *result, void *aligned_out, size_t out_stride);
int rsreg_gicp6d_align_cloud(rsreg_ctx *ctx, const float *guess, const rsreg_gicp_params *params, double lab_weight,
                             rsreg_gicp_result *result, rsreg_cloud *aligned_out);

/* ---- pcl::transformPointCloud(in, out, Matrix4f) ------------------------------------ */
/* incremental_icp.hpp:63, icp_edge...hpp:116-117, ndt_edge...hpp:104-105.  in == out is
 * allowed.  Records are copied whole (stride bytes) and xyz rewritten; when !is_dense,
 * non-finite points are copied unchanged. */
int rsreg_transform_cloud(rsreg_ctx *ctx, const void *in, void *out, size_t n, size_t stride,
                          int is_dense, const float transform[16]);

/* ---- pcl::ApproximateVoxelGrid<PointXYZRGB>::filter --------------------------------- */
/* incremental_icp.hpp:54-55, icp_edge...hpp:47,59-60,75-76, ndt_edge...hpp:45,57-58,68-69.
 * Order-dependent streaming hash-history centroiding; this entry point runs it sequentially
 * on the host (no context needed), record for record like PCL.  Records must be PointXYZRGB (stride >= 20, rgb
 * at byte 16).  out must hold n records; *n_out receives the count.  in == out allowed.
 * The contract, the same for this entry point, the GPU filter and the oracle (float32, one IEEE operation at a time):
 * (1) The stream: a history of 512 slots.  A record whose slot holds another voxel flushes that voxel's centroid to the
 *     output and takes the slot; at the end the occupied slots are flushed in slot order.
 * (2) The centroid: the sums of x, y, z and of the r, g, b bytes (each converted to float first), from +0.0f on in input
 *     order, divided by (float)count.  The colour is (int) of the three byte means, r << 16 | g << 8 | b; the fourth float is
 *     1.0f; everything else in the record is zero.
 * (3) A record with a non-finite x, y or z takes no part.
 * (4) The cell index of a coordinate: c = floorf(x * inv) with inv = 1.0f / leaf; it is INT32_MIN when c is a NaN or
 *     outside [-2^31, 2^31), otherwise the integer c.  That is what the conversion delivers on x86, and therefore what PCL
 *     computes there; every implementation here writes it out.  So a leaf whose reciprocal is +inf is accepted (every cell
 *     index of that axis is INT32_MIN), and coordinates of either sign past int32 share one voxel.
 * (5) The slot: (ix * 7171 + iy * 3079 + iz * 4231) modulo 2^32, & 511. */
int rsreg_approx_voxel_grid(const void *in, size_t n, size_t stride, const float leaf[3],
                            void *out, size_t *n_out);
/* The same filter on the GPU, same output record for record: the points of one hash slot are
 * an independent stream, each run of equal voxels in it gives one centroid (float sums in input
 * order), and a run is emitted where the next run of its slot begins -- all of which sorts and
 * scans reconstruct (csrc/voxel.hip).  stride must be a multiple of 4. */
int rsreg_approx_voxel_grid_gpu(rsreg_ctx *ctx, const void *in, size_t n, size_t stride,
                                const float leaf[3], void *out, size_t *n_out);

/* ---- pcl::VoxelGrid<PointXYZRGB>::filter: one centroid per occupied leaf, in leaf order ---------------------------------
 * The downsampler in front of NormalEstimation and IterativeClosestPointWithNormals; the reference's pre-filter declares a
 * cloud_voxel_grid it never fills (src/capture.hpp:112-132).  PCL is not available to check against: what follows is
 * recalled from PCL 1.9.1, filters/impl/voxel_grid.hpp and common/impl/centroid.hpp, and IS the contract.  All arithmetic is
 * float32, one IEEE operation at a time (no contracted multiply-add); float -> int32 conversions saturate (a leaf coordinate
 * past int32 is outside what PCL defines).
 * (1) A record with a non-finite x, y or z takes no part: not in the box, not in a leaf, not in a count -- whatever is_dense
 *     says (PCL's behaviour on a cloud flagged dense that holds NaNs is undefined).
 * (2) Box: min_p, max_p = the componentwise minimum and maximum over the finite records; inv[a] = 1.0f / leaf[a];
 *     d[a] = (int64)((max_p[a] - min_p[a]) * inv[a]) + 1.  If d[0] * d[1] * d[2] > INT32_MAX (PCL: "leaf size is too small",
 *     output = input) the output is a copy of the input: all records, the input's width, height and is_dense, and
 *     info->overflowed = 1 with every box field of info zero.
 * (3) Leaf of a point p: min_b[a] = (int)floorf(min_p[a] * inv[a]), max_b likewise from max_p; div_b = max_b - min_b + 1;
 *     divb_mul = (1, div_b[0], div_b[0] * div_b[1]); ijk[a] = (int)(floorf(p[a] * inv[a]) - (float)min_b[a]);
 *     idx = ijk . divb_mul as an unsigned 32-bit value (products and sums modulo 2^32, as div_b and divb_mul are).
 * (4) The output's leaves are in ascending idx.
 * (5) A leaf's points are added in ascending input index.  STATED CHOICE: PCL's std::sort leaves the order inside a leaf
 *     unspecified; this is the only point on which the result can differ from a PCL build.
 * (6) A leaf with fewer than min_points_per_voxel points gives no output (default 0).
 * (7) downsample_all_data = 1 (PCL's default, its CentroidPoint): float sums of x, y, z and of the r, g, b, a bytes (each
 *     converted to float before it is added); xyz = sum / (float)n; each colour byte = (uint32_t)(sum / (float)n), packed
 *     a << 24 | r << 16 | g << 8 | b.  (ApproximateVoxelGrid leaves alpha 0; here it is averaged.)
 * (8) downsample_all_data = 0: xyz from the same sums, the colour PCL's default (r = g = b = 0, a = 255).
 * (9) An output record is a zeroed record of the input's stride (>= 20, a multiple of 4, rgb at byte 16) with xyz, 1.0f in
 *     the fourth float (both modes: a default-constructed point) and the colour set.  width = leaves kept, height = 1,
 *     is_dense = 1.  An empty or all-non-finite input gives an empty output.
 * A leaf that is not positive, not finite, or whose reciprocal is not finite: RSREG_ERR_INVALID_ARG.
 * NOT BUILT: the filter-field limits (setFilterFieldName / setFilterLimits: run rsreg_cloud_passthrough first) and the saved
 * leaf layout (setSaveLeafLayout, getCentroidIndex). */
typedef struct rsreg_voxel_grid_params {
    float leaf[3];
    int downsample_all_data;
    uint32_t min_points_per_voxel;
} rsreg_voxel_grid_params;
/* getMinBoxCoordinates, getMaxBoxCoordinates, getNrDivisions, getDivisionMultiplier of the last filter() and its counts */
typedef struct rsreg_voxel_grid_info {
    int32_t min_b[3], max_b[3], div_b[3], divb_mul[3];
    uint64_t n_finite, n_leaves, n_out;   /* finite records; occupied leaves; records in the output */
    int overflowed;
} rsreg_voxel_grid_info;
/* PCL's defaults: downsample_all_data = 1, min_points_per_voxel = 0; the leaf is unset (0: refused until it is set) */
void rsreg_voxel_grid_params_default(rsreg_voxel_grid_params *params);
/* The contract restated sequentially on the host (no context needed).  out must hold n records; in == out allowed. */
int rsreg_voxel_grid(const void *in, size_t n, size_t stride, const float leaf[3], int downsample_all_data,
                     uint32_t min_points, void *out, size_t *n_out, rsreg_voxel_grid_info *info /* may be NULL */);
/* The same on the GPU, the same bytes (csrc/voxel.hip): the box, a stable radix sort of the records by leaf index over
 * exactly the key bits the box needs, and per leaf the float sums in input order by the run kernels of the approximate
 * filter.  No float atomics; the same bytes from any context. */
int rsreg_voxel_grid_gpu(rsreg_ctx *ctx, const void *in, size_t n, size_t stride, const rsreg_voxel_grid_params *params,
                         void *out, size_t *n_out, rsreg_voxel_grid_info *info /* may be NULL */);

/* ---- NDT: pcl::NormalDistributionsTransform<PointXYZRGB,PointXYZRGB> ---------------- */
/* ndt.setInputTarget (ndt_edge...hpp:72): voxel binning + per-voxel mean / covariance /
 * regularised inverse covariance (VoxelGridCovariance). */
int rsreg_ndt_set_target(rsreg_ctx *ctx, const void *points, size_t n, size_t stride,
                         int is_dense, double resolution);
/* ndt.setInputSource + ndt.align(out, guess) + getFinalTransformation
 * (ndt_edge...hpp:71,83,92,104). */
int rsreg_ndt_align(rsreg_ctx *ctx, const void *source, size_t n, size_t stride, int is_dense,
                    const float *guess, const rsreg_ndt_params *params, rsreg_ndt_result *result,
                    void *aligned_out, size_t out_stride);
/* One score/gradient/Hessian pass at pose p = [tx ty tz rx ry rz] (tests; the unit an
 * N-GPU run all-reduces; on the wire 1 + 6 + 21 doubles, the Hessian being symmetric). */
int rsreg_ndt_derivatives(rsreg_ctx *ctx, const void *source, size_t n, size_t stride,
                          int is_dense, const double pose[6], double *score, double gradient[6],
                          double hessian[36]);
/* Which point a voxel is searched by (VoxelGridCovariance's centroid cloud, ndt_edge_based_registration.hpp:71-72 ->
 * setInputTarget).  0 (default): the voxel's f64 mean rounded to float.  1: PCL's own arithmetic -- a float running
 * sum over the voxel's points in input order, divided by float(n) (voxel_grid_covariance.hpp: leaf.centroid += pt;
 * leaf.centroid /= nr_points) -- one sequential chain per voxel, for bit-level agreement with a PCL build.  Applies
 * to the targets set afterwards.  Optionally reads the centroids back (3 floats per valid voxel). */
int rsreg_ndt_set_centroid_mode(rsreg_ctx *ctx, int mode);
int rsreg_ndt_get_centroids(rsreg_ctx *ctx, float *centroids /*3 each*/, int32_t capacity);
/* Read back the valid voxels: per voxel 3 (mean) + 9 (cov) + 9 (icov) doubles and a count. */
int rsreg_ndt_get_voxels(rsreg_ctx *ctx, int32_t *n_voxels, double *mean_cov_icov /*21 each*/,
                         int32_t *counts, int32_t capacity);

/* ---- N-GPU: one pair sharded by source-point blocks --------------------------------- */
/* One process per GPU.  Rank 0 calls rsreg_comm_unique_id, the caller ships the 128 bytes
 * to every rank (any side channel, e.g. torch.distributed broadcast over gloo), every rank
 * calls rsreg_comm_init.  After that rsreg_icp_align / rsreg_ndt_align all-reduce their
 * sums (17 / 28 doubles per pass: NDT ships the score, the gradient and the upper triangle
 * of the Hessian) over RCCL on the ctx stream; every rank then runs the
 * same host solve on identical numbers, so no broadcast of the transform is needed. */
#define RSREG_UNIQUE_ID_BYTES 128
int rsreg_comm_unique_id(uint8_t id[RSREG_UNIQUE_ID_BYTES]);
int rsreg_comm_init(rsreg_ctx *ctx, const uint8_t id[RSREG_UNIQUE_ID_BYTES], int rank, int nranks);
int rsreg_comm_destroy(rsreg_ctx *ctx);
/* All-reduce (sum) `count` doubles in place across the ranks of ctx's communicator. */
int rsreg_comm_allreduce_f64(rsreg_ctx *ctx, double *host_buf, int count);

/* ---- device-resident clouds: the frame loop without leaving HBM ------------------------- */
/* The reference's schemes run, per frame, ApproximateVoxelGrid::filter -> align (-> align) ->
 * transformPointCloud x2 -> operator+ on host clouds (incremental_icp.hpp:54-64,
 * icp_edge_based_registration.hpp:75-76,95-120, ndt_edge_based_registration.hpp:68-108).  A
 * rsreg_cloud holds the records of one cloud in HBM (whole records, `stride` bytes each, plus
 * width / height / is_dense); every step below takes and leaves its clouds there, so a frame is
 * uploaded once and the merged cloud downloaded once.  A cloud belongs to the ctx it was created
 * on; handles given to rsreg_icp_set_*_cloud must stay alive and unchanged until the align that
 * uses them has returned. */
int rsreg_cloud_create(rsreg_ctx *ctx, rsreg_cloud **out);
int rsreg_cloud_destroy(rsreg_cloud *cloud);
int rsreg_cloud_upload(rsreg_cloud *cloud, const void *points, size_t n, size_t stride, uint32_t width,
                       uint32_t height, int is_dense);
/* The same, returning as soon as the records are staged: the PCIe copy runs on a copy stream of the context beside the
 * work of the main stream (a frame loop uploads frame k + 1 while frame k is being aligned: incremental_icp.hpp:51-66
 * hands over all frames up front).  Every call that reads or rewrites the cloud waits for the copy first; `points` may
 * be reused when the call returns. */
int rsreg_cloud_upload_async(rsreg_cloud *cloud, const void *points, size_t n, size_t stride, uint32_t width,
                             uint32_t height, int is_dense);
/* rsreg_cloud_upload_async that returns before `points` has been read: the records are staged and their copy queued by a
 * thread of the context.  `points` must stay valid and unchanged until a call that reads or rewrites the cloud (any of
 * them waits for the upload) has returned.  For callers whose frames stay put for the whole registration -- the
 * reference's schemes take the caller's vector of clouds (types.hpp:19) and read frame k + 2 while frame k is aligned. */
int rsreg_cloud_upload_deferred(rsreg_cloud *cloud, const void *points, size_t n, size_t stride, uint32_t width,
                                uint32_t height, int is_dense);
int rsreg_cloud_download(const rsreg_cloud *cloud, void *out, size_t capacity_records);
/* rsreg_cloud_download that returns at once: the records as they are when the context's stream gets here go to `out`
 * (capacity in records) on a download stream and the copy-out threads of the context; the cloud may be rewritten or
 * destroyed right away.  `out` must stay valid and untouched until rsreg_ctx_wait_downloads(ctx) has returned.  The frame
 * loops hand every frame's moved points to the host this way while the next frames are aligned (the merged cloud the
 * schemes return, types.hpp:19, is then complete when the loop ends: incremental_icp.hpp:63-64, icp_edge...hpp:116-120). */
int rsreg_cloud_download_async(const rsreg_cloud *cloud, void *out, size_t capacity_records);
int rsreg_ctx_wait_downloads(rsreg_ctx *ctx);
int rsreg_cloud_info(const rsreg_cloud *cloud, size_t *n, size_t *stride, uint32_t *width, uint32_t *height,
                     int *is_dense);
const void *rsreg_cloud_device_ptr(const rsreg_cloud *cloud);
/* Which cloud this is (`id`, unique per handle) and how often its records have been rewritten (`version`: every upload,
 * filter, transform, concatenation or alignment INTO the handle counts).  A host layer that keeps PCL's
 * "setInputSource once, align many times" habit compares the pair with what it loaded last and loads again when the
 * cloud has changed in place in between (pcl_compat.hpp; PCL itself would see the new points through its pointer:
 * incremental_icp.hpp:57-59 sets both inputs before every align anyway). */
int rsreg_cloud_version(const rsreg_cloud *cloud, uint64_t *id, uint64_t *version);
int rsreg_cloud_copy(rsreg_ctx *ctx, const rsreg_cloud *in, rsreg_cloud *out);
/* ApproximateVoxelGrid::filter, same records in the same order as the host filter; in == out allowed */
int rsreg_cloud_filter(rsreg_ctx *ctx, const rsreg_cloud *in, const float leaf[3], rsreg_cloud *out);
/* The same queued by a thread of the context on a stream and scratch of its own: returns at once; the number of output
 * records is known, and the records are there, when a call that takes `out` has waited for them (every one does).  The
 * frame loops filter the next frames this way while they align this one (incremental_icp.hpp:54-55 filters every frame
 * independently of the registration).  `in` must stay alive and unchanged until `out` has been used; in != out.  `in`
 * may be the output of rsreg_cloud_edge_features_async that has not run yet: the jobs run in the order of the calls. */
int rsreg_cloud_filter_async(rsreg_ctx *ctx, const rsreg_cloud *in, const float leaf[3], rsreg_cloud *out);
/* pcl::VoxelGrid::filter on a device cloud ("pcl::VoxelGrid" above is the contract); in == out allowed; `out` follows the
 * versioning rules (its version changes, except that an overflowed filter of a cloud into itself leaves it as it is).
 * Waits for the stream: once for the box, once for the number of leaves, once more when min_points_per_voxel > 1. */
int rsreg_cloud_voxel_grid(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_voxel_grid_params *params, rsreg_cloud *out,
                           rsreg_voxel_grid_info *info /* may be NULL */);
/* pcl::transformPointCloud; in == out allowed */
int rsreg_cloud_transform(rsreg_ctx *ctx, const rsreg_cloud *in, const float transform[16], rsreg_cloud *out);
/* PointCloud::operator+ : out = a followed by b (width = size, height = 1, is_dense = both); out may be a or b */
int rsreg_cloud_concat(rsreg_ctx *ctx, const rsreg_cloud *a, const rsreg_cloud *b, rsreg_cloud *out);
/* ---- cloud filters: the reference's pre-filter (src/capture.hpp:112-132, filter_pcl: PassThrough on z, then
 * StatisticalOutlierRemoval with setMeanK(50), setStddevMulThresh(1.5)).  On the context's stream; `out` follows the
 * versioning rules above (its version changes); in == out allowed.
 *
 * pcl::PassThrough (filters/impl/passthrough.hpp, PCL 1.9.1, recalled): field 0 = x, 1 = y, 2 = z.  A record with a non-finite
 * x, y or z is removed; otherwise it is removed when v < lo || v > hi (negative: when lo <= v <= hi), float compares.  Kept
 * records keep their order and all their bytes; out: width = kept, height = 1, is_dense = 1.  keep_organized: nothing is
 * dropped, a removed record gets x = y = z = quiet NaN, width / height are the input's, is_dense = 0 if anything was
 * removed.  Any other field: RSREG_ERR_INVALID_ARG (PCL warns and returns an empty cloud). */
int rsreg_cloud_passthrough(rsreg_ctx *ctx, const rsreg_cloud *in, int field, float lo, float hi, int negative,
                            int keep_organized, rsreg_cloud *out);
/* pcl::StatisticalOutlierRemoval (filters/impl/statistical_outlier_removal.hpp, recalled) with an EXACT k-nearest-neighbour
 * search over the finite records: distance = (float)(sum of the mean_k smallest non-self float distances, added in
 * ascending order in double, / mean_k); a non-finite record has distance 0 and is kept unless `negative`;
 * threshold = mean + stddev_mult * stddev over the distances (sums over all records, divided by n_valid); a record is
 * removed when distance > threshold (negative: when distance <= threshold).  out: width = kept, height = 1, is_dense as
 * the input's.  mean_k: 1 .. 64, RSREG_ERR_INVALID_ARG above (never an approximation); RSREG_ERR_INVALID_ARG too when
 * the cloud has fewer than mean_k + 1 finite records (PCL reads past its arrays) or fewer than 2 (PCL divides by zero).
 * Waits for the stream (the number of kept records). */
typedef struct rsreg_sor_stats {
    uint64_t n_valid, n_kept;   /* finite records; records in `out` */
    double mean, stddev, threshold;
} rsreg_sor_stats;
int rsreg_cloud_sor(rsreg_ctx *ctx, const rsreg_cloud *in, int mean_k, double stddev_mult, int negative, rsreg_cloud *out,
                    rsreg_sor_stats *stats /* may be NULL */);
/* The first pass of rsreg_cloud_sor on its own: host_out[i] = record i's distance (n floats, the caller's record order) */
int rsreg_cloud_knn_mean_distance(rsreg_ctx *ctx, const rsreg_cloud *in, int mean_k, float *host_out);
/* nearestKSearch of every record in its own cloud, EXACT: for every finite record the k finite records with the smallest
 * float32 L2_Simple squared distances, the record itself and exact copies counted like any other; ascending by
 * (d2, original record index), and among records whose d2 equals the k-th smallest value the lowest indices (the tie
 * rule of every search here).  1 <= k <= 64; fewer than k finite records: RSREG_ERR_INVALID_ARG.  Host outputs, each nullable.
 * The range of every exact search here (this one, the mean distances, the radius search, getFitnessScore): any finite float32
 * coordinates, of the cloud and, for getFitnessScore, of the source however far outside the target's box.  A squared distance that overflows is +inf and ties with every other +inf (lowest index first; a mean over one is
 * +inf), one in the float32 denormals keeps the bits IEEE arithmetic gives it, one that underflows is 0.
 * index_out:    n*k int32 original record indices, ascending (d2, index); a non-finite record's row is all -1.
 * sqr_dist_out: n*k float; a non-finite record's row is all 0. */
int rsreg_cloud_knn(rsreg_ctx *ctx, const rsreg_cloud *in, int k, int32_t *index_out, float *sqr_dist_out);
/* pcl::NormalEstimation with setKSearch(k), 3 <= k <= 64; viewpoint NULL = (0,0,0).
 * out: n records of 32 bytes laid out as pcl::Normal: normal_x, normal_y, normal_z, 0.f, curvature, 0, 0, 0.
 * width, height as the input's.  out != in.
 * Over the k neighbours of rsreg_cloud_knn: C = (sum d d^T) / k - (sum d / k)(sum d / k)^T with d = neighbour - record in
 * double, summed in a fixed order; normal = the unit eigenvector of C's smallest eigenvalue l0 (Jacobi, double), rounded to
 * float; curvature = (float)|l0 / (l0 + l1 + l2)|, 0 when the trace is 0 (solvePlaneParameters); flipped when, with
 * v = viewpoint - record in float, (v.x * nx + v.y * ny) + v.z * nz < 0 (flipNormalTowardsViewpoint).  All k neighbours in
 * one place (trace 0): (0, 0, 1) before the flip, curvature 0.  A non-finite record gets four quiet NaNs (normal and
 * curvature); if any record did, out's is_dense is 0, otherwise the input's.  Fewer than k finite records:
 * RSREG_ERR_INVALID_ARG.  The same cloud gives the same bytes whatever the context has indexed before.
 * DEVIATION FROM PCL 1.9.1, stated: PCL accumulates nine raw moments about the origin in float, in FLANN's neighbour order
 * (computeMeanAndCovarianceMatrix); this is the covariance the formula defines, in double, about the record.  A PCL build
 * agrees with it to PCL's own rounding. */
int rsreg_cloud_normals(rsreg_ctx *ctx, const rsreg_cloud *in, int k, const float viewpoint[3], rsreg_cloud *out);
/* ---- pcl::FPFHEstimation with setKSearch(k), 2 <= k <= 64: the Simplified Point Feature Histogram of every record and the Fast
 * Point Feature Histogram weighted from them.  PCL 1.9.1 features/impl/fpfh.hpp (computePointSPFHSignature,
 * weightPointSPFHSignature) and pfh_tools.cpp (computePairFeatures), recalled; PCL is not available to check against, so what
 * follows IS the contract.
 * normals: n records (the same n as `in`, the same context), normal_x, normal_y, normal_z the first three floats of each, stride
 * >= 12 and a multiple of 4: what rsreg_cloud_normals wrote is accepted as it is.  Another size or context, k outside 2 .. 64,
 * fewer than k finite records: RSREG_ERR_INVALID_ARG, nothing launched.
 * Neighbourhood N(i): the k neighbours of rsreg_cloud_knn, ascending by (d2, index), the record itself among them; d2(i, .) their
 * float32 squared distances.
 * Pair features of record i and neighbour j, in DOUBLE from the float inputs, no contraction.  Skipped when j == i.
 *   dp = p_j - p_i; f4 = sqrt((dp.x^2 + dp.y^2) + dp.z^2); skipped when f4 == 0.
 *   a1 = (n_i . dp) / f4, a2 = (n_j . dp) / f4, every dot product here summed as (x + y) + z.
 *   fabs(a1) < fabs(a2): n1 = n_j, n2 = n_i, dp = -dp, f3 = -a2; otherwise n1 = n_i, n2 = n_j, f3 = a1.  (PCL's
 *   acos(fabs(a1)) > acos(fabs(a2)), without the acos.)
 *   v = dp x n1 = (dp.y n1.z - dp.z n1.y, dp.z n1.x - dp.x n1.z, dp.x n1.y - dp.y n1.x); |v| = sqrt((v.x^2 + v.y^2) + v.z^2);
 *   skipped when |v| == 0; v = v / |v| (three divisions).
 *   w = n1 x v (the same component formula); f2 = v . n2; f1 = atan2(w . n2, n1 . n2).
 *   Skipped when n_i or n_j is not finite (a stated choice: PCL's behaviour there is undefined).
 * Bins, 11 per feature: floor of 11 * ((f1 + pi) * (1 / (2 pi))), 11 * ((f2 + 1) * 0.5), 11 * ((f3 + 1) * 0.5), each clamped to
 * [0, 10].
 * SPFH row of record i: 33 floats, feature 1 first.  A bin hit by c pairs holds the float that adding
 * hist_incr = 100.0f / (float)(k - 1) to 0.0f c times gives (PCL's sequential +=; the increments are equal, so the value depends
 * on c alone).  A skipped pair adds nothing and hist_incr still uses k - 1.  A record that is not finite, or whose normal is not
 * finite, has an all-zero row.
 * FPFH row of record i, in float32, no contraction, in PCL's order:
 *   for a in 0 .. k-1 (neighbour order): if d2[a] == 0 continue (the record itself, exact copies); w = 1.0f / d2[a];
 *     for t in 0 .. 2: for b in 0 .. 10: val = SPFH[N(i)[a]][t][b] * w; sum_t += val; h[t][b] += val;
 *   for t in 0 .. 2: if (sum_t != 0) sum_t = (float)(100.0 / (double)sum_t); h[t][b] *= sum_t.
 * Two quirks of PCL are kept: the weight is 1 / SQUARED distance, and the record's own SPFH does not enter its FPFH.  A record
 * with no neighbour at positive distance gives 33 zeros, never a division by zero.  A record that is not finite, or whose own
 * normal is not finite, gets 33 quiet NaNs.  A finite record can get NaNs by the arithmetic above as well, when 1.0f / d2[a] or a
 * product overflows (a denormal d2 gives w = +inf, and 0 * inf is NaN): the NaNs stand where the formula puts them, their sign
 * and payload are not specified, and is_dense is 0 as for any other NaN.
 * DEVIATION FROM PCL 1.9.1, stated: PCL computes the pair features in float through Eigen; here they are computed in double.  A PCL
 * build can differ where a feature lies within float rounding of a bin edge.
 * The same cloud, normals and k give the same bytes whatever the context has indexed before: the counts are integers, every
 * float sum runs in the order above.
 * Not built: setSearchSurface with setKSearch, setIndices, other bin counts, PFH.  setRadiusSearch: rsreg_cloud_fpfh_radius,
 * below; setSearchSurface with it: rsreg_cloud_fpfh_radius_surface.
 *
 * rsreg_cloud_fpfh: out = n records of 132 bytes laid out as pcl::FPFHSignature33 (float histogram[33]); width, height as the
 * input's; is_dense 0 if any record got NaNs, otherwise the input's.  out != in, out != normals.  Waits for the stream (whether a
 * record got NaNs).
 * rsreg_cloud_spfh: host_out = the n * 33 floats of the SPFH rows, the caller's record order. */
int rsreg_cloud_fpfh(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, int k, rsreg_cloud *out);
int rsreg_cloud_spfh(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, int k, float *host_out /* n*33 */);
/* ---- feature matching: the exact k-nearest-neighbour search of one cloud's descriptors among another cloud's, and
 * pcl::registration::CorrespondenceEstimation<FPFHSignature33, FPFHSignature33> over it (determineCorrespondences,
 * determineReciprocalCorrespondences).  PCL 1.9.1 registration/impl/correspondence_estimation.hpp, KdTreeFLANN and FLANN's
 * L2_Simple<float>, recalled; PCL is not available to check against, so what follows IS the contract.
 * A DESCRIPTOR CLOUD is a device cloud whose records start with 33 floats: stride >= 132 and a multiple of 4.  What
 * rsreg_cloud_fpfh wrote is accepted as it is, and so are wider records with a payload behind the row, which nothing reads.  A row
 * is VALID when all 33 floats are finite (DefaultPointRepresentation::isValid).
 * Distance of source row s and target row t, float32, sequential in bin order, no contraction:
 *   d2 = 0.0f; for b in 0 .. 32: diff = s[b] - t[b]; d2 += diff * diff.
 * A sum that overflows is +inf, which ties with every other +inf.
 * The search is exact: bit-equal to a brute force in that order, ties to the lowest target index, and the same bytes whatever the
 * context has done before -- every pair is computed, the selection is a minimum of unique (d2, index) keys.
 *
 * rsreg_cloud_feature_knn: for every valid source row the k valid target rows with the smallest d2, ascending by (d2, target
 * record index); among rows whose d2 equals the k-th smallest the lowest indices win.  Host outputs, ns * k each, each nullable; an
 * invalid source row gets indices -1 and distances 0 (the convention of rsreg_cloud_knn).  1 <= k <= 16.  RSREG_ERR_INVALID_ARG with
 * nothing searched and the outputs untouched: fewer than k valid target rows (the pass that counts them is all that has run), k out
 * of range, a NULL cloud, a cloud of another context, a stride under 132 or not a multiple of 4, an empty source.  source == target is allowed: a row then finds itself, or a
 * lower-indexed exact copy, at d2 = 0.  Waits for the stream.
 *
 * rsreg_correspondence: pcl::Correspondence, 12 bytes; distance is the SQUARED distance, as in PCL.
 * rsreg_cloud_feature_correspondences:
 *   max_dist_sqr = max_distance * max_distance in double: DBL_MAX gives +inf, which keeps everything.  max_distance negative or
 *   NaN: RSREG_ERR_INVALID_ARG.
 *   For every valid source row i in ascending order: j = its nearest valid target row (k = 1 as above), d2 their distance.  The row
 *   is dropped when (double)d2 > max_dist_sqr -- a distance AT the bound is kept -- otherwise {i, j, d2} is emitted.
 *   reciprocal != 0: i' = the nearest valid SOURCE row of target row j, d2' its distance, the same tie rule.  The row is also
 *   dropped when (double)d2' > max_dist_sqr || i' != i.
 *   The output is ordered by index_query.  *n_out = the number found; when it exceeds `capacity` the first `capacity` are written
 *   and the call still returns RSREG_OK: the caller sees *n_out > capacity, nothing is hidden.  host_out may be NULL when capacity
 *   is 0.  No valid target row, or (reciprocal) no valid source row, or an empty cloud: *n_out = 0, RSREG_OK.  Waits for the stream.
 * Not built: setIndices, descriptors of other lengths, other metrics.  What turns the list into a pose is the next section. */
typedef struct rsreg_correspondence {
    int32_t index_query;   /* source row */
    int32_t index_match;   /* target row */
    float distance;        /* squared */
} rsreg_correspondence;
int rsreg_cloud_feature_knn(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, int k, int32_t *index_out /* ns*k */,
                            float *sqr_dist_out /* ns*k */);
int rsreg_cloud_feature_correspondences(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, double max_distance, int reciprocal,
                                        rsreg_correspondence *host_out, size_t capacity, size_t *n_out);
/* ---- pose from correspondences: pcl::registration::CorrespondenceRejectorSampleConsensus (RANSAC over a correspondence list, its
 * model pcl::SampleConsensusModelRegistration) and pcl::registration::TransformationEstimationSVD over a correspondence list.  PCL
 * 1.9.1 registration/impl/correspondence_rejection_sample_consensus.hpp, sample_consensus/impl/sac_model_registration.hpp and
 * sample_consensus/impl/ransac.hpp, recalled; PCL is not available to check against, so what follows IS the contract, and where it
 * leaves PCL it says DEVIATION.
 * Inputs of every entry point: two device clouds of the context whose records start with x, y, z floats (stride >= 12 and a multiple
 * of 4; source == target is allowed) and a HOST array of n rsreg_correspondence: index_query names a source record, index_match a
 * target record, distance is ignored.  An index outside its cloud, a NULL cloud, a cloud of another context or such a stride:
 * RSREG_ERR_INVALID_ARG, checked on the host before anything is launched.  The list goes to the device once a call and is gathered
 * into six coordinate planes there.  A pair is FINITE when its six coordinates are.  All calls wait for the stream.
 * The score of one pair (p the source point, q the target point) under a transform T (m = its rows), float32, every operation rounded
 * once, no contraction:
 *   p'.x = ((m0[0] * p.x + m0[1] * p.y) + m0[2] * p.z) + m0[3], p'.y and p'.z alike (transformPointCloud's order);
 *   dx = p'.x - q.x, ...; d2 = (dx * dx + dy * dy) + dz * dz (L2_Simple, as every search here).
 * The pair is an INLIER iff it is finite and (double)d2 < threshold * threshold: strictly, as in PCL's countWithinDistance.  NaN
 * compares false.  threshold negative or NaN: RSREG_ERR_INVALID_ARG.  Every float32 operation is IEEE: denormals are kept, an
 * overflow is +-inf and inf - inf is NaN.  threshold * threshold is a double product: when it is +inf or above FLT_MAX every finite
 * pair with a finite d2 is an inlier, when it is at most 2^-149 only d2 == 0 is, and when it is 0 (a threshold below 1.5e-162) none.
 *
 * rsreg_cloud_count_inliers: counts_out[h] = the inliers of transforms[16 * h .. 16 * h + 15] (column-major 4 x 4, host; the last
 *   row is not read), h < H.  Any floats are allowed in a transform; a pair whose d2 is NaN or +inf is not an inlier.  H == 0: nothing
 *   is written.  n == 0: zeros.
 *
 * rsreg_cloud_estimate_rigid_svd: TransformationEstimationSVD::estimateRigidTransformation(source, target, correspondences).
 *   sums_out = the RSREG_NUM_SUMS sums of the finite pairs in the layout above ([0] their number, [1..3] sum p, [4..6] sum q,
 *   [7 + 3 r + c] sum q[r] * p[c], [16] sum of d2 of the pairs as they stand, d2 the float32 L2_Simple of p and q), in double.  The
 *   products of two floats are exact in double; the additions run in a fixed tree that is a function of n alone: pair i is term
 *   i % 64 of wave (i / 64) % 2 of group i / 128; a wave's 64 terms meet pairwise across lane bit 5, 4, 3, 2, 1, 0; a group is wave 0 +
 *   wave 1; groups g, g + 256, g + 512, .. are added in ascending order into one of 256 strands, strand t meets strands t + 32, + 16, ..,
 *   + 1 within its 64, and the four 64s are added in order.  A pair that is not finite, or left out, is a term of +0.
 *   t_out is exactly rsreg_umeyama_from_sums(sums_out).  Fewer than three finite pairs: RSREG_ERR_INVALID_ARG.  Either output may be NULL.
 *
 * rsreg_cloud_sac_correspondences: the rejector.  params NULL: rsreg_sac_params_default (PCL's defaults: inlier_threshold 0.05,
 *   max_iterations 1000, probability 0.99; refit_rounds 0, min_sample_distance 0, seed 0).  probability outside (0, 1),
 *   min_sample_distance negative or NaN, max_iterations or refit_rounds negative: RSREG_ERR_INVALID_ARG.
 *   HYPOTHESIS h (h = 0, 1, ...) draws from a counter-based generator, all in uint64 arithmetic modulo 2^64:
 *     z = seed + (64 * h + draw) * 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     z = z ^ (z >> 31); index(h, draw) = ((z >> 32) * n) >> 32.
 *   Try t = 0 .. 15 takes the pairs i0, i1, i2 = index(h, 3 t), index(h, 3 t + 1), index(h, 3 t + 2).  The try is GOOD when the three
 *   indices differ, the three pairs are finite, the three source points are pairwise apart by (double)d2 > min_sample_distance^2 (d2
 *   their float32 L2_Simple; with 0 this refuses coincident points), and rsreg_umeyama_from_sums succeeds on the three pairs' sums
 *   (double, each sum 0.0 + the term of i0 + that of i1 + that of i2).  The first good try gives the hypothesis its T; sixteen bad
 *   tries make it INVALID: its count is 0 and the stopping rule passes over it.
 *   The d2 of two source points is a float32 like any other: a cloud whose squared point distances underflow float32 (points less
 *   than about 2^-75 apart, denormal clouds) has no valid sample at min_sample_distance 0 and the call reports NO MODEL after one
 *   iteration; a d2 that overflowed to +inf is above the square of every min_sample_distance whose own square is finite.
 *   DEVIATION: PCL's rand()-driven sampler, its isSampleGood threshold derived from the cloud's covariance and its skipped-sample
 *   counter are not reproduced; min_sample_distance is the explicit stand-in for that threshold.
 *   count[h] = the inliers of T(h) at inlier_threshold.
 *   THE STOPPING RULE is PCL's (ransac.hpp), replayed sequentially in double over the counts:
 *     k = 1; best = -1 (PCL's -INT_MAX: the first valid hypothesis always sets k); for h = 0, 1, .. while h < k and h < max_iterations:
 *       if h is valid and count[h] > best: best = count[h]; winner = h; w = (double)best / (double)n; q = 1 - w * w * w;
 *         q = min(max(q, DBL_EPSILON), 1 - DBL_EPSILON); k = log(1 - probability) / log(q).
 *   The device scores the hypotheses in batches and may score more than the replay consumes; the result does not depend on the batches.
 *   DEVIATION: PCL's iterations_ > max_iterations_ off-by-one (one more iteration than asked) is not kept.
 *   The winner is the FIRST h that reached the final best.  NO MODEL when n < 3 or best < 3: found = 0, transform the identity,
 *   best_hypothesis and sample -1, n_inliers 0, and all n correspondences remain (host_out = the input list) -- what PCL does when
 *   computeModel fails.
 *   Otherwise transform = T(winner), the kept pairs are its inliers, and refit_rounds = r refits up to r times: T = the fit of
 *   rsreg_cloud_estimate_rigid_svd over the current inliers -- the tree of the WHOLE list, every pair that is not an inlier a term of
 *   +0 in its place -- (a round does not start with fewer than three), then the inliers are
 *   selected again under T; the rounds end early when no pair's flag changed.  DEVIATION: this is not PCL's refineModel (its
 *   variance-driven threshold loop is not built).
 *   host_out: the kept correspondences in input order, their records unchanged.  *n_out = their number; when it exceeds `capacity`
 *   the first `capacity` are written and the call still returns RSREG_OK (the convention of rsreg_cloud_feature_correspondences).
 *   Every output is a function of the two clouds, the list and the parameters alone: the counts are integers, the generator is a
 *   function of (seed, h, draw), every float sum has its order written above.
 * Not built: the other CorrespondenceRejector*, refineModel.  (SampleConsensusPrerejective and SampleConsensusInitialAlignment: the two
 * sections after this one.) */
typedef struct rsreg_sac_params {
    double inlier_threshold;      /* 0.05 */
    double probability;           /* 0.99 */
    double min_sample_distance;   /* 0 */
    int32_t max_iterations;       /* 1000 */
    int32_t refit_rounds;         /* 0 */
    uint64_t seed;                /* 0 */
} rsreg_sac_params;
typedef struct rsreg_sac_result {
    float transform[16];          /* column-major */
    int32_t found;
    int32_t best_hypothesis;
    int32_t sample[3];            /* the winner's three pairs (positions in the input list) */
    int32_t iterations;           /* hypotheses the replay consumed */
    uint64_t n_inliers;
    int32_t refit_rounds_run;
    int32_t reserved0;
    double sums[RSREG_NUM_SUMS];  /* the last refit's sums; zeros when there was none */
} rsreg_sac_result;
void rsreg_sac_params_default(rsreg_sac_params *p);
int rsreg_cloud_count_inliers(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const rsreg_correspondence *corr, size_t n,
                              const float *transforms /* H*16 */, size_t H, double threshold, uint32_t *counts_out /* H */);
int rsreg_cloud_estimate_rigid_svd(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const rsreg_correspondence *corr, size_t n,
                                   float t_out[16], double sums_out[RSREG_NUM_SUMS]);
int rsreg_cloud_sac_correspondences(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const rsreg_correspondence *corr, size_t n,
                                    const rsreg_sac_params *params /* may be NULL */, rsreg_correspondence *host_out, size_t capacity, size_t *n_out,
                                    rsreg_sac_result *result /* may be NULL */);
/* ---- pose from descriptor neighbours: pcl::SampleConsensusPrerejective -- three source records, each paired with a random one of
 * its k nearest descriptors, a cheap edge-length test (pcl::registration::CorrespondenceRejectorPoly), and the surviving poses scored
 * against the WHOLE target cloud by a nearest-point search.  PCL 1.9.1 registration/impl/sample_consensus_prerejective.hpp and
 * correspondence_rejection_poly.hpp, recalled; PCL is not available to check against, so what follows IS the contract, and where it
 * leaves PCL it says DEVIATION.
 * Inputs of both entry points: two device clouds of the context whose records start with x, y, z floats (stride >= 12 and a multiple
 * of 4; source == target is allowed).  A NULL cloud, a cloud of another context or such a stride: RSREG_ERR_INVALID_ARG.  Both calls
 * index the target once (a round trip to the host for its box) and wait for the stream.
 *
 * THE SCORE of a transform T (m = its rows) over the source: for every source record i whose x, y, z are finite,
 *   p' = the float32 transform of the pair score above: p'.x = ((m0[0] * p.x + m0[1] * p.y) + m0[2] * p.z) + m0[3], p'.y and p'.z
 *   alike (transformPointCloud's order), every operation rounded once, no contraction;
 *   if p' is finite, d2 = the EXACT nearest float32 L2_Simple squared distance from p' to the finite target records, d2 = the
 *   minimum over the target records q of (dx * dx + dy * dy) + dz * dz with dx = p'.x - q.x, ... (the search of getFitnessScore);
 *   the record is an INLIER iff (double)d2 < max_range * max_range: strictly, PCL's getFitness.  The product is a double: when it is
 *   +inf or above FLT_MAX every record with a finite d2 is an inlier, when it is at most 2^-149 only d2 == 0 is, and when it is 0 none.
 *   A record that is not finite, a p' that is not finite, a d2 that is +inf or NaN, an empty or all-non-finite target: no inlier.
 * count = the number of inliers.  sum = the sum of the inliers' d2 in double, in a tree that is a function of the source's record
 * count ns alone: record i is term i % 64 of wave (i / 64) % 2 of group i / 128; a record that is not an inlier is a term of +0.0,
 * and so is every term behind record ns - 1 of the last group; a wave's 64 terms meet pairwise across lane bit 5, 4, 3, 2, 1, 0
 * (term t + term t + 32, then those 32 sums t + t + 16, ..); a group is wave 0 + wave 1; the groups are added in ascending order,
 * starting from group 0's value: ((g0 + g1) + g2) + ...  No float atomics anywhere: the same clouds, transforms and range give the
 * same bytes for any batch, slice, launch order or context.
 *
 * rsreg_cloud_score_transforms: the scoring stage on its own, the counterpart of rsreg_cloud_count_inliers with a search in place of
 *   a list.  counts_out[h] and sums_out[h] = the count and the sum of transforms[16 * h .. 16 * h + 15] (column-major 4 x 4, host; the
 *   last row is not read), h < H; either may be NULL.  Any floats are allowed in a transform.  H == 0: nothing is written.  An empty
 *   source, an empty or all-non-finite target: zeros.  max_range negative or NaN: RSREG_ERR_INVALID_ARG.
 *
 * rsreg_cloud_prerejective: neighbor_index is a HOST table of ns rows of k int32, exactly what
 *   rsreg_cloud_feature_knn(source_features, target_features, k) wrote: row i holds the k target records nearest to source record i in
 *   descriptor space; a row of -1 makes record i INELIGIBLE.  1 <= k <= 16.  An entry >= nt, a negative one other than -1, or a row
 *   that is -1 only in part: RSREG_ERR_INVALID_ARG, checked on the host before anything is launched.  The table (ns * k * 4 bytes) goes
 *   to the device once a call; a device-resident table is not built.
 *   params NULL: rsreg_prerej_params_default (similarity_threshold 0.9, inlier_fraction 0, select_by_inliers 0, seed 0; max_iterations
 *   10 and max_correspondence_distance sqrt(DBL_MAX), pcl::Registration's own defaults).  max_iterations negative,
 *   similarity_threshold outside [0, 1) or NaN, inlier_fraction outside [0, 1] or NaN, max_correspondence_distance negative or NaN:
 *   RSREG_ERR_INVALID_ARG.  DEVIATION: nr_samples is 3 and nothing else (setNumberOfSamples is not built).
 *   HYPOTHESIS h, h = 0 .. max_iterations - 1, makes ONE try (PCL's iteration: a rejected sample spends its iteration), with the
 *   generator of the section above, index(h, draw, n) = ((z >> 32) * n) >> 32 over z = the splitmix64 finaliser of
 *   seed + (64 * h + draw) * 0x9E3779B97F4A7C15: s_d = index(h, d, ns) for d = 0, 1, 2 are its source records, and
 *   t_d = neighbor_index[s_d * k + index(h, 3 + d, k)] their target records.
 *   h is VALID when s_0, s_1, s_2 differ, each is eligible, all six points are finite, the polygon test passes and
 *   rsreg_umeyama_from_sums succeeds on the three pairs' sums (double, each sum 0.0 + the term of pair 0 + that of pair 1 + that of
 *   pair 2, as the rejector above forms them); T(h) is that solve's result.
 *   THE POLYGON TEST, float32: for each of the three edges (a, b), ds = the L2_Simple squared distance of source points a and b, dt
 *   that of their target points; sim = ds < dt ? ds / dt : dt / ds, one IEEE float32 division; the edge passes iff
 *   sim >= similarity_threshold * similarity_threshold, the product rounded to float32.  A NaN sim, which 0 / 0 gives, fails: coincident
 *   points are refused without a further rule.  A denormal ds or dt is divided as IEEE: nothing is flushed to zero.  A cloud whose
 *   squared edge lengths all underflow to 0 (0 / 0), or overflow to +inf (inf / inf, a NaN as well), has no valid hypothesis.  At
 *   similarity_threshold 0 an edge with exactly one zero length passes (sim = 0 / x = 0 >= 0): three source records matched to ONE
 *   target record then reach the solve, which decides.
 *   DEVIATION: PCL's rand()-driven sampler is not reproduced.
 *   A valid hypothesis is scored as above at max_range = max_correspondence_distance; an invalid one is never searched.
 *   SELECTION, replayed on the host in hypothesis order: h QUALIFIES when it is valid, count >= 1 and
 *   (double)count / (double)ns >= inlier_fraction, ns EVERY source record (input_->size()); error = sum / count in double.
 *   select_by_inliers == 0: the winner is the first h with the strictly lowest error among the qualifying (PCL's error < lowest_error).
 *   DEVIATION: PCL keeps the error in float and accumulates the fitness in float in point order.
 *   select_by_inliers == 1, an EXTENSION: the winner is the qualifying h with the highest count, then the lowest error, then the lowest
 *   h.  PCL's rule with inlier_fraction 0 crowns any three-point pose whose samples happen to sit on target points (a count of 3
 *   and an error near 0 beats every better-supported pose); this rule is what asks for support first.
 *   No early stop (PCL 1.9.1 has none): every h < max_iterations is generated, and the result does not depend on the batches.
 *   result: found = 0 when no hypothesis qualifies (also: an empty cloud, max_iterations 0): transform the identity, n_inliers 0,
 *   fitness 0, best_hypothesis, sample and match -1, *n_out = 0.  Otherwise transform = T(winner), sample / match its s_d / t_d,
 *   n_inliers its count, fitness its error.  n_valid: the valid hypotheses, i.e. the ones that were scored.
 *   inliers_out: the winner's inlier source records in ascending order.  *n_out = their number; when it exceeds `capacity` the first
 *   `capacity` are written and the call still returns RSREG_OK (the convention of rsreg_cloud_feature_correspondences).  inliers_out
 *   may be NULL when capacity is 0.
 *   Every output is a function of the two clouds, the table and the parameters alone.
 * Not built: a device-resident neighbour table, a refit over the winner's inliers.  (SampleConsensusInitialAlignment, which takes
 * nr_samples up to 8: the section after this one; this estimator stays at 3.) */
typedef struct rsreg_prerej_params {
    double max_correspondence_distance;   /* sqrt(DBL_MAX) */
    double inlier_fraction;               /* 0 */
    float similarity_threshold;           /* 0.9 */
    int32_t max_iterations;               /* 10 */
    int32_t select_by_inliers;            /* 0: PCL's rule */
    int32_t reserved0;
    uint64_t seed;                        /* 0 */
} rsreg_prerej_params;
typedef struct rsreg_prerej_result {
    float transform[16];                  /* column-major */
    int32_t found;
    int32_t best_hypothesis;
    int32_t sample[3];                    /* the winner's three source records */
    int32_t match[3];                     /* ... and their target records */
    uint64_t n_valid;                     /* hypotheses that were scored */
    uint64_t n_inliers;
    double fitness;                       /* the winner's error: sum / count */
} rsreg_prerej_result;
void rsreg_prerej_params_default(rsreg_prerej_params *p);
int rsreg_cloud_score_transforms(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const float *transforms /* H*16 */, size_t H,
                                 double max_range, uint32_t *counts_out /* H, may be NULL */, double *sums_out /* H, may be NULL */);
int rsreg_cloud_prerejective(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const int32_t *neighbor_index /* ns*k */, int k,
                             const rsreg_prerej_params *params /* may be NULL */, int32_t *inliers_out, size_t capacity, size_t *n_out,
                             rsreg_prerej_result *result /* may be NULL */);
/* ---- pose from descriptor neighbours, scored by a robust error: pcl::SampleConsensusInitialAlignment (SAC-IA), the estimator FPFH was
 * published with -- nr_samples source records that keep a minimum distance from one another, each paired with a random one of its k
 * nearest descriptors; NO hypothesis is thrown away, every one is scored over EVERY source record by a bounded penalty of its
 * nearest-point distance.  PCL 1.9.1 registration/impl/ia_ransac.hpp and ia_ransac.h, recalled; PCL is not available to check against,
 * so what follows IS the contract, and where it leaves PCL it says DEVIATION.
 * Inputs: those of rsreg_cloud_prerejective -- two device clouds of the context (records that start with x, y, z floats; source ==
 *   target is allowed) and, where a call takes one, the HOST table neighbor_index of ns rows of k int32 that
 *   rsreg_cloud_feature_knn(source_features, target_features, k) wrote, 1 <= k <= 16 (PCL's k_correspondences_, default 10), a row of -1
 *   making its record INELIGIBLE.  The same checks, the same refusals (RSREG_ERR_INVALID_ARG before anything is launched).  Every call
 *   that searches indexes the target once (the prerejective build) and every call waits for the stream.
 * params NULL: rsreg_scia_params_default.
 *   max_correspondence_distance (default sqrt(DBL_MAX)): thr = (float) of it.  PCL'S QUIRK, KEPT: thr is compared with the SQUARED
 *     distance (the PCL tutorial passes 0.01f * 0.01f).  thr NaN or <= 0: RSREG_ERR_INVALID_ARG; +inf is allowed (the default is +inf
 *     as a float).
 *   min_sample_distance (default 0): negative or NaN: RSREG_ERR_INVALID_ARG.
 *   nr_samples (default 3): outside 3 .. 8: RSREG_ERR_INVALID_ARG.
 *   error_function: RSREG_SCIA_TRUNCATED (PCL's default) or RSREG_SCIA_HUBER; anything else: RSREG_ERR_INVALID_ARG.
 *   max_iterations (default 10, pcl::Registration's own): negative: RSREG_ERR_INVALID_ARG.  seed (default 0).
 *
 * THE ERROR of a transform T over the source: for every source record whose x, y, z are finite, p' = the float32 transform of the
 *   sections above (transformPointCloud's order, every operation rounded once, no contraction); e = the EXACT nearest float32
 *   L2_Simple squared distance from p' to the finite target records (the search of rsreg_cloud_score_transforms); e = +inf when p'
 *   is not finite, when the target has no finite record, or when the nearest distance overflowed.
 *   The record's term, TruncatedError: (e < +inf && e <= thr) ? (double)(e / thr) : 1.0 -- one IEEE float32 division, nothing flushed
 *     (a denormal thr divides as IEEE; thr = +inf gives +0 for every finite e).
 *   HuberPenalty, in double without contraction, e and thr converted exactly: e <= thr ? (0.5 * e) * e : (0.5 * thr) * (2.0 * e - thr);
 *     +inf for e = +inf.  (PCL's functors take the squared distance as written here: the quirk above.)
 *   A source record that is not finite is a term of +0.0.
 *   error = the sum of the terms in double, in exactly the tree of the section above: record i is term i % 64 of wave (i / 64) % 2 of
 *   group i / 128, +0.0 behind record ns - 1; a wave's 64 terms meet pairwise across lane bit 5, 4, 3, 2, 1, 0; a group is wave 0 +
 *   wave 1; the groups are added in ascending order starting from group 0's value.  The tree is a function of ns alone.
 *   DEVIATION: PCL adds the terms in float in point order.
 *   With the truncated term the search may stop at thr (nothing farther changes the term); with Huber it is unbounded.
 *
 * rsreg_cloud_error_transforms: the scoring stage on its own, the counterpart of rsreg_cloud_score_transforms.  errors_out[h] = the
 *   error of transforms[16 * h .. 16 * h + 15] (column-major 4 x 4, host; the last row is not read), h < H.  Any floats are allowed in a
 *   transform.  H == 0: nothing is written.  An empty source: zeros.  An empty or all-non-finite target: every finite source record
 *   has e = +inf.  thr and error_function are checked as above.
 *
 * HYPOTHESIS h uses the generator of the sections above: index(h, draw, n) = ((z >> 32) * n) >> 32 over z = the splitmix64 finaliser
 *   of seed + (64 * h + draw) * 0x9E3779B97F4A7C15.
 *   THE SAMPLER: the candidate draws d = 0 .. 55 give c = index(h, d, ns), taken in order.  A candidate is ACCEPTED when its row is
 *   eligible, its record is finite, it differs from every accepted sample, and for every accepted sample s
 *   (double)d2(c, s) >= min_sample_distance * min_sample_distance (a double product), d2 the float32 L2_Simple of the two source
 *   points: at min_sample_distance 0 coincident records pass and the solve decides.  DEVIATION: PCL compares a float sqrt.
 *   The first nr_samples accepted candidates are s_0, s_1, ..; fewer after the 56 draws: the hypothesis is INVALID.
 *   DEVIATION: PCL halves min_sample_distance_ after 3 * ns failures and KEEPS the halved value for the rest of the call; this is not
 *   reproduced -- n_valid tells the caller how many hypotheses found a sample.  ns < nr_samples: nothing is valid.
 *   Target records: t_j = neighbor_index[s_j * k + index(h, 56 + j, k)], j < nr_samples.
 *   h is VALID when the sampler filled, every t_j is finite and rsreg_umeyama_from_sums succeeds on the pairs' sums (double, each
 *   sum 0.0 + the term of pair 0 + that of pair 1 + .., as the sections above form them); T(h) is that solve's result.
 *   A valid hypothesis is ALWAYS scored; an invalid one is never searched.  DEVIATION: rand() is not reproduced.
 *
 * rsreg_cloud_initial_alignment_hypotheses: the sampler and the fit alone, for hypotheses first .. first + count - 1 (params gives
 *   seed, nr_samples and min_sample_distance; every field is checked as above).  Per hypothesis: transforms_out 16 floats (column-major,
 *   last row 0 0 0 1; sixteen quiet NaNs when it is invalid), valid_out one int32 (1 / 0), samples_out 16 int32: s_0 .. in [0, 8),
 *   t_0 .. in [8, 16), -1 behind nr_samples, -1 x 16 when the sampler did not fill.  Each output may be NULL.  The rows do not depend
 *   on `first` and `count`: hypothesis h is a function of (seed, h).
 *
 * rsreg_cloud_initial_alignment: SELECTION is replayed on the host in hypothesis order, PCL's `i_iter == 0 || error < lowest_error`
 *   in double.  guess (a column-major 4 x 4, may be NULL; the last row is not read): the guess is scored first, whatever
 *   max_iterations is, and spends one iteration: the hypotheses are h = 0 .. H - 1 with H = max(max_iterations - 1, 0); without a guess
 *   H = max_iterations.  DEVIATION: PCL's guess.isApprox(Identity, 0.01) test is replaced by NULL.
 *   A guess whose error is not NaN holds lowest_error.  The valid hypotheses follow in order: while nothing holds lowest_error the
 *   first whose error is not NaN takes it (+inf included); afterwards one takes it iff its error is strictly lower.  The winner is
 *   thus the first valid h with the strictly lowest error; a NaN error never wins.
 *   errors_out (may be NULL): max_iterations doubles; [h] = the error of hypothesis h, quiet NaN for an invalid one and for the
 *   places h >= H.
 *   result: found is PCL's converged_: 1 only when a hypothesis won (not the guess); then transform = T(winner), best_hypothesis = h,
 *   sample / match = its s_j / t_j (-1 behind nr_samples), error = its error.  Otherwise best_hypothesis, sample and match are -1,
 *   the transform is the guess if there is one and its error is finite (the guess's 16 floats as given), the identity if not, and
 *   error = the guess's error, +inf when nothing was scored.  n_valid: the valid hypotheses, i.e. the ones that were scored.  An empty
 *   source: nothing is scored.  No early stop: every h < H is generated.
 * Determinism: every output is a function of the two clouds, the table and the parameters alone: the same bytes for any batch, slice,
 *   launch order or context; no float atomics anywhere.
 * Not built: PCL's persistent relaxation of min_sample_distance, setIndices, a device-resident neighbour table. */
typedef enum rsreg_scia_error_function {
    RSREG_SCIA_TRUNCATED = 0,             /* pcl::SampleConsensusInitialAlignment::TruncatedError, PCL's default */
    RSREG_SCIA_HUBER = 1                  /* ... ::HuberPenalty */
} rsreg_scia_error_function;
typedef struct rsreg_scia_params {
    double max_correspondence_distance;   /* sqrt(DBL_MAX); compared, as a float, with the SQUARED distance */
    double min_sample_distance;           /* 0 */
    int32_t nr_samples;                   /* 3; 3 .. 8 */
    int32_t error_function;               /* RSREG_SCIA_TRUNCATED */
    int32_t max_iterations;               /* 10 */
    int32_t reserved0;
    uint64_t seed;                        /* 0 */
} rsreg_scia_params;
typedef struct rsreg_scia_result {
    float transform[16];                  /* column-major */
    int32_t found;                        /* a hypothesis won */
    int32_t best_hypothesis;
    int32_t sample[8];                    /* the winner's source records, -1 behind nr_samples */
    int32_t match[8];                     /* ... and their target records */
    uint64_t n_valid;                     /* hypotheses that were scored */
    double error;                         /* the winner's (or the guess's) error; +inf when nothing was scored */
} rsreg_scia_result;
void rsreg_scia_params_default(rsreg_scia_params *p);
int rsreg_cloud_error_transforms(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const float *transforms /* H*16 */, size_t H,
                                 int error_function, double max_correspondence_distance, double *errors_out /* H */);
int rsreg_cloud_initial_alignment_hypotheses(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const int32_t *neighbor_index /* ns*k */,
                                             int k, const rsreg_scia_params *params /* may be NULL */, uint64_t first, size_t count,
                                             float *transforms_out /* count*16 */, int32_t *valid_out /* count */, int32_t *samples_out /* count*16 */);
int rsreg_cloud_initial_alignment(rsreg_ctx *ctx, const rsreg_cloud *source, const rsreg_cloud *target, const int32_t *neighbor_index /* ns*k */, int k,
                                  const rsreg_scia_params *params /* may be NULL */, const float *guess /* 16, may be NULL */,
                                  double *errors_out /* max_iterations, may be NULL */, rsreg_scia_result *result /* may be NULL */);
/* ---- radius search: every record's neighbours within a radius in its own cloud, EXACT.  Record j is a neighbour of the finite
 * record i when j is finite and d2(i, j) < r2, with d2 the float32 L2_Simple squared distance of every search here and
 * r2 = (float)((double)radius * (double)radius): KdTreeFLANN::radiusSearch's cast and the STRICT compare of FLANN's
 * RadiusResultSet::addPoint, both recalled from PCL 1.9.1 / FLANN -- neither is available to check against, so this IS the
 * contract.  The record itself and exact copies are neighbours like any other; a record AT the radius is not one.  No cap on the
 * number of neighbours.  radius not finite or <= 0: RSREG_ERR_INVALID_ARG.  Every call builds its index (a round trip to the host
 * for the box).
 *
 * host_out[i] = record i's number of neighbours (n uint32, the caller's record order): >= 1 for a finite record (itself), 0 for a
 * non-finite one. */
int rsreg_cloud_radius_count(rsreg_ctx *ctx, const rsreg_cloud *in, double radius, uint32_t *host_out);
/* pcl::RadiusOutlierRemoval (filters/impl/radius_outlier_removal.hpp, PCL 1.9.1, recalled): with count as above a record is
 * removed when count <= min_neighbors (negative: when count > min_neighbors); a non-finite record goes by the same rule with its
 * count of 0.  Kept records keep their order and all their bytes; out: width = kept, height = 1, is_dense as the input's.
 * keep_organized: nothing is dropped, a removed record gets x = y = z = quiet NaN, width / height are the input's, is_dense = 0
 * if anything was removed.  in == out allowed; `out` follows the versioning rules above.  *n_kept: the records kept.
 * min_neighbors < 0: RSREG_ERR_INVALID_ARG.  Waits for the stream (the number of kept records).
 * DEVIATION FROM PCL 1.9.1, stated: on a dense cloud PCL takes a k-nearest-neighbour shortcut and compares the
 * (min_neighbors + 1)-th squared distance against r2 with `>`, which differs from the rule above only for a record at exactly
 * the radius; here the one rule holds for every cloud. */
int rsreg_cloud_radius_outlier_removal(rsreg_ctx *ctx, const rsreg_cloud *in, double radius, int min_neighbors, int negative,
                                       int keep_organized, rsreg_cloud *out, uint64_t *n_kept /* may be NULL */);
/* pcl::NormalEstimation with setRadiusSearch(radius); viewpoint NULL = (0,0,0).  out: n pcl::Normal records as
 * rsreg_cloud_normals writes them, width, height as the input's; out != in.
 * Over the m neighbours within the radius (above): C = (sum d d^T) / m - (sum d / m)(sum d / m)^T with d = neighbour - record in
 * double, then eigenvector, curvature, flip and the trace-0 case exactly as rsreg_cloud_normals.  m < 3: four quiet NaNs (PCL's
 * computePointNormal returns false below three points).  A non-finite record gets four quiet NaNs; if any record got NaNs, out's
 * is_dense is 0, otherwise the input's.  The sums run in an order that is a function of the cloud and the radius alone (inside
 * a cell of the index the points lie in ascending record index): the same cloud gives the same bytes whatever the context has
 * indexed before.  Waits for the stream (whether a record got NaNs).
 * DEVIATION FROM PCL 1.9.1, stated: PCL accumulates nine raw moments about the origin in float, in FLANN's neighbour order
 * (computeMeanAndCovarianceMatrix); this is the covariance the formula defines, in double, about the record.  A PCL build
 * agrees with it to PCL's own rounding. */
int rsreg_cloud_normals_radius(rsreg_ctx *ctx, const rsreg_cloud *in, double radius, const float viewpoint[3], rsreg_cloud *out);
/* ---- pcl::ISSKeypoint3D (Intrinsic Shape Signatures) over the radius search above: the keypoint detector in front of the
 * descriptors.  PCL 1.9.1 keypoints/impl/iss_3d.hpp (getScatterMatrix, detectKeypoints), recalled; PCL is not available to check
 * against, so what follows IS the contract.
 * Neighbourhood: both radii use the neighbourhood of rsreg_cloud_radius_count, unchanged -- record j is a neighbour of the finite
 *   record i when j is finite and float32 d2(i, j) < (float)((double)r * (double)r), strictly; the record itself and exact copies
 *   among them; no cap.  m_s(i), m_n(i): the counts at the salient and at the non-max radius.
 * Scatter (PCL's getScatterMatrix, recalled): S = sum d d^T over the m_s neighbours, d = (double)neighbour - (double)record, in
 *   double without contraction; not divided, not centred.  The sums run in the order of the index, a function of the cloud and
 *   the SALIENT radius alone (inside a cell the points lie in ascending record index): what rsreg_cloud_normals_radius states.
 *   m_s < min_neighbors: S stays zero.
 * Eigenvalues: l1 >= l2 >= l3 of S by the f64 cyclic Jacobi of rsreg_cloud_normals; eig_out holds them ASCENDING, three per
 *   record; a non-finite record, and one below min_neighbors, gets zeros.
 *   DEVIATION FROM PCL 1.9.1, stated: PCL runs Eigen's SelfAdjointEigenSolver; a PCL build agrees to the rounding of the solve.
 * Saliency (PCL's third_eigen_value_): 0 unless all three values are finite, l3 >= 0, l2 / l1 < gamma_21 and l3 / l2 < gamma_32
 *   (IEEE double divisions; a NaN ratio fails its compare); otherwise l3.
 * Non-maximum suppression: record i is a keypoint iff saliency[i] > 0, m_n(i) >= min_neighbors, and no neighbour j within the
 *   non-max radius has saliency[i] < saliency[j].  The compare is strict: exact ties all remain.  rsreg_cloud_iss_non_max takes
 *   the CALLER'S saliencies and compares them as written: a NaN is never above 0 and never exceeds anything, a negative value is
 *   never a keypoint and never suppresses a positive one, +inf is allowed.
 * Output: the keypoints in ascending record index.  out (may be NULL): their records with every byte kept, width = n_keypoints,
 *   height = 1, is_dense = 1; out != in; `out` follows the versioning rules above.  index_out (may be NULL): the first `capacity`
 *   of the same indices (PCL's getKeypointsIndices); *n_keypoints (may be NULL) is their full number and may exceed capacity.
 * ONE INDEX: rsreg_cloud_iss_keypoints builds the index once, at the salient radius, and walks it a second time with the non-max
 *   radius -- the reach of a walk is taken from the actual cell, so a radius above or below the cell stays exact (a non-max radius
 *   far below the salient one reads more candidates than an index of its own would).  rsreg_cloud_iss_non_max indexes at its radius.
 * Refused with RSREG_ERR_INVALID_ARG, nothing launched and `out` untouched: a radius that is not finite or <= 0 (rsreg_cloud_iss_saliency
 *   does not read non_max_radius), min_neighbors < 0, a gamma that is not finite, out == in, a null `in`, params, saliency or
 *   is_keypoint_out, a cloud of another context.  An empty cloud, or one without a finite record: zero keypoints, zero rows.
 * Determinism: the same cloud and parameters give the same bytes from any context, whatever it has indexed before.
 * Every call waits for the stream.
 * Not built: border estimation (setBorderRadius / setNormalRadius / setAngleThreshold with BoundaryEstimation), setIndices,
 *   setSearchSurface, the other keypoint detectors (Harris3D, SIFT, NARF, ...). */
typedef struct rsreg_iss_params {
    double salient_radius;    /* setSalientRadius: > 0, finite */
    double non_max_radius;    /* setNonMaxRadius:  > 0, finite */
    double gamma_21;          /* setThreshold21, PCL default 0.975 */
    double gamma_32;          /* setThreshold32, PCL default 0.975 */
    int32_t min_neighbors;    /* setMinNeighbors, PCL default 5; >= 0 */
    int32_t reserved;         /* 0 */
} rsreg_iss_params;
void rsreg_iss_params_default(rsreg_iss_params *p);   /* gammas 0.975, min_neighbors 5, radii 0 (refused until set) */
int rsreg_cloud_iss_saliency(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_iss_params *params, double *eig_out /* n*3, may be NULL */,
                             double *saliency_out /* n, may be NULL */, uint32_t *count_out /* n, may be NULL */);
int rsreg_cloud_iss_non_max(rsreg_ctx *ctx, const rsreg_cloud *in, const double *saliency /* n, host */, double non_max_radius,
                            int min_neighbors, uint8_t *is_keypoint_out /* n */);
int rsreg_cloud_iss_keypoints(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_iss_params *params, rsreg_cloud *out /* may be NULL */,
                              int32_t *index_out /* capacity entries, may be NULL */, size_t capacity, uint64_t *n_keypoints /* may be NULL */);
/* ---- pcl::EuclideanClusterExtraction over the radius search above: a cloud split into its connected pieces.  PCL 1.9.1
 * segmentation/impl/extract_clusters.hpp (extractEuclideanClusters), recalled; PCL is not available to check against, so what
 * follows IS the contract.
 * Graph: the nodes are the finite records of the cloud.  Records i != j are joined when float32 d2(i, j) < r2, strictly, with
 *   r2 = (float)((double)tolerance * (double)tolerance): the neighbourhood of rsreg_cloud_radius_count, unchanged, and symmetric
 *   because L2_Simple is.  Exact copies are joined like any other pair; a record AT the tolerance is not joined.
 * Cluster: a connected component of this graph whose number of records m satisfies min_cluster_size <= m <= max_cluster_size.  A
 *   component outside the bounds is dropped whole, never split (PCL compares the finished seed queue with both bounds).
 * Order: the clusters are ranked by size descending (PCL's std::sort(clusters.rbegin(), clusters.rend(), comparePointClusters));
 *   inside a cluster the record indices ascend (PCL's std::sort on r.indices).
 *   DEVIATIONS FROM PCL 1.9.1, stated: PCL's unstable sort leaves the order of equal sizes open -- here a tie goes to the cluster
 *   whose smallest record index is lower.  A non-finite record belongs to no cluster -- PCL's seed loop would make it a singleton
 *   when min_cluster_size <= 1.
 * rsreg_cloud_euclidean_clusters, every output in host memory and nullable:
 *   labels_out[i] (n): the rank of record i's cluster, 0 the largest; -1 for a non-finite record and for one of a dropped component.
 *   indices_out (n): the record indices of cluster 0 ascending, then those of cluster 1, ...; entries beyond the last reported
 *     cluster are not written.
 *   offsets_out (min(n_clusters, capacity) + 1): offsets_out[c] .. offsets_out[c + 1] is cluster c's slice of indices_out.  Only the
 *     first `capacity` clusters are reported.
 *   *n_clusters_out: always the full number of clusters, which may exceed capacity.
 *   An empty cloud, or one without a finite record: 0 clusters, offsets_out[0] = 0, every label -1, no kernel of the clustering runs.
 * rsreg_cloud_cluster_filter, the consumer that stays on the device: keeps the records whose cluster rank lies in
 *   [rank_lo, rank_hi) (negative: the others; a record with label -1 is outside every range).  (0, 1): the largest cluster only;
 *   (0, UINT32_MAX) with a min_cluster_size: every blob below that size dropped.  out, in == out, keep_organized, is_dense, the
 *   versioning and *n_kept are those of rsreg_cloud_radius_outlier_removal, through the same flag / scan / gather kernels.
 * The result is a function of the cloud and the parameters alone: a component's representative is its smallest record index
 *   whatever order the device linked the edges in, and the ranks are a total order.  The same bytes from any context.
 * Refused with RSREG_ERR_INVALID_ARG, nothing written and `out` unchanged: a tolerance that is not finite or <= 0,
 *   min_cluster_size > max_cluster_size, rank_lo > rank_hi, a NULL p, in or out, a cloud of another context, 2^30 records or more.
 * Both calls build the index (a round trip to the host for the box) and wait for the stream.
 * Not built: setIndices and setSearchMethod, LabeledEuclideanClusterExtraction, ConditionalEuclideanClustering, RegionGrowing,
 *   clustering across ranks (every rank clusters the cloud it holds). */
typedef struct rsreg_cluster_params {
    double tolerance;            /* setClusterTolerance; must be finite and > 0 */
    uint32_t min_cluster_size;   /* setMinClusterSize, PCL default 1 */
    uint32_t max_cluster_size;   /* setMaxClusterSize, PCL default INT_MAX */
} rsreg_cluster_params;
void rsreg_cluster_params_default(rsreg_cluster_params *p);   /* tolerance 0: the caller must set it */
int rsreg_cloud_euclidean_clusters(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cluster_params *p, int32_t *labels_out /* n, may be NULL */,
                                   uint32_t *indices_out /* n, may be NULL */, uint32_t *offsets_out /* min(n_clusters, capacity) + 1, may be NULL */,
                                   uint32_t capacity, uint32_t *n_clusters_out /* may be NULL */);
int rsreg_cloud_cluster_filter(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cluster_params *p, uint32_t rank_lo, uint32_t rank_hi, int negative,
                               int keep_organized, rsreg_cloud *out, uint64_t *n_kept /* may be NULL */);
/* ---- plane segmentation: pcl::SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE and SAC_RANSAC -- the dominant
 * plane of a cloud (floor, table, wall) -- and pcl::ExtractIndices to consume its result: the step in front of
 * EuclideanClusterExtraction.  PCL 1.9.1 sample_consensus/impl/sac_model_plane.hpp, sac_model_perpendicular_plane.hpp, ransac.hpp and
 * segmentation/impl/sac_segmentation.hpp, recalled; PCL is not available to check against, so what follows IS the contract, and
 * where it leaves PCL it says DEVIATION.
 * Inputs of every entry point: one device cloud of the context whose records start with x, y, z floats (stride >= 12 and a multiple
 * of 4).  A NULL cloud, a cloud of another context or such a stride: RSREG_ERR_INVALID_ARG, nothing written (the refusals of the
 * other cloud operations).  A record is FINITE when its three coordinates are.  n = the records of the cloud.  All calls wait for
 * the stream.
 * The distance of a record p to a model (a, b, c, d), float32, every operation rounded once, no contraction:
 *   dist = ((a * p.x + b * p.y) + c * p.z) + d.
 * p is an INLIER iff it is finite and (double)fabsf(dist) < threshold: strictly.  NaN compares false.  (Implemented as
 * fabsf(dist) < thr_up with thr_up the least float >= threshold, which is the same predicate.)  threshold negative or NaN:
 * RSREG_ERR_INVALID_ARG; 0 is allowed and admits nothing.  Every float32 operation is IEEE: denormals are kept, an overflow is
 * +-inf and inf - inf is NaN.  Any four floats are allowed as a model in rsreg_cloud_plane_count and rsreg_cloud_plane_filter -- a
 * zero normal, NaN and inf included; a record whose dist is NaN or +-inf is not an inlier.
 *
 * HYPOTHESIS h (h = 0, 1, ...) draws record indices with the generator of rsreg_cloud_sac_correspondences, unchanged: index(h, draw)
 *   as written there, with n the number of records.  Try t = 0 .. 15 takes the records i0, i1, i2 = index(h, 3 t), index(h, 3 t + 1),
 *   index(h, 3 t + 2), with points p0, p1, p2.  The try is GOOD when the three indices differ, the three records are finite, and with
 *   (float32; each product rounded, then the subtraction)
 *     u = p1 - p0; v = p2 - p0; nx = u.y * v.z - u.z * v.y; ny = u.z * v.x - u.x * v.z; nz = u.x * v.y - u.y * v.x;
 *     n2 = (nx * nx + ny * ny) + nz * nz
 *   n2 is finite and > 0.  The first good try gives the model: l = sqrtf(n2); a = nx / l; b = ny / l; c = nz / l (sqrt and divide
 *   correctly rounded); d = -((a * p0.x + b * p0.y) + c * p0.z).  Fewer than three records: no try is good.
 *   DEVIATION: PCL's rand()-driven sampler and its ratio test for collinear samples are not reproduced.
 *   THE AXIS CONSTRAINT (SACMODEL_PERPENDICULAR_PLANE) applies when eps_angle > 0 and the axis is not zero.  In double, each written
 *   operation rounded once, a, b, c the floats above and (ax, ay, az) the axis:
 *     cs = |(a * ax + b * ay) + c * az| / (sqrt((a * a + b * b) + c * c) * sqrt((ax * ax + ay * ay) + az * az)).
 *   The model passes iff cs >= cos_eps, with cos_eps = std::cos(eps_angle) computed once on the host and returned in the result.
 *   DEVIATION: PCL compares acos angles.
 *   A hypothesis is VALID when it has a good try and, where the constraint applies, its model passes it; otherwise it is INVALID and
 *   its count is 0.  count[h] = the inliers of model(h) at distance_threshold.
 * THE STOPPING RULE is PCL's (ransac.hpp), this time with its skip counter (the axis constraint makes invalid hypotheses the common
 *   case, and a rule that spent an iteration on each would stop after hypothesis 0), replayed sequentially in double over h = 0, 1, ..:
 *     it = 0; skipped = 0; k = 1; best = -1; while it < k and it < max_iterations and skipped < 10 * max_iterations:
 *       h invalid: ++skipped, nothing else.
 *       h valid: if count[h] > best: best = count[h]; winner = h; w = (double)best / (double)n; q = 1 - w * w * w;
 *         q = min(max(q, DBL_EPSILON), 1 - DBL_EPSILON); k = log(1 - probability) / log(q).  Then ++it.
 *   DEVIATION: PCL's iterations_ > max_iterations_ off-by-one is not kept (as in rsreg_cloud_sac_correspondences).
 *   The device scores the hypotheses in batches (at most 11 * max_iterations in all) and may score more than the replay consumes;
 *   the result does not depend on the batches.  The winner is the FIRST h that reached the final best.
 *   NO MODEL when n < 3 or best < 3: found = 0, the coefficients are zeros, best_hypothesis and sample are -1, there are no inliers.
 *   Refused with RSREG_ERR_INVALID_ARG: probability outside (0, 1), max_iterations negative, eps_angle negative or NaN, an axis that
 *   is not finite, distance_threshold negative or NaN.
 * REFINEMENT (optimize_coefficients, on by default as in PCL) runs over the winner's inliers.  Ten double sums are taken of
 *   e = (double)p - (double)p0, p0 the winner's first sample record (RSREG_NUM_PLANE_SEG_SUMS): [0] the number of inliers m,
 *   [1..3] sum e, [4..9] sum of e.x e.x, e.x e.y, e.x e.z, e.y e.y, e.y e.z, e.z e.z (each product a double product, rounded once).
 *   They are added in the tree written out for rsreg_cloud_estimate_rigid_svd: term i is record i, and a record that is not an
 *   inlier is a term of +0.  rsreg_plane_from_sums (host only, no ctx) turns them into a model:
 *     mean = sum e / m; C = sum e e^T / m - mean mean^T; the normal is the unit eigenvector of C's smallest eigenvalue (cyclic Jacobi
 *     in double); its sign is chosen so that its dot product with the prior model's (a, b, c) is >= 0; a, b, c are its components
 *     rounded to float; d = (float)(-normal . (p0 + mean)), in double.
 *   It returns RSREG_ERR_INVALID_ARG and writes nothing when m < 3 or C is not finite.  The inliers are then selected again under the
 *   refined model (PCL does the same).  With fewer than 3 inliers, or when rsreg_plane_from_sums refuses, the unrefined model is
 *   kept; `refined` says which model the result holds.
 *   DEVIATION: PCL accumulates the covariance in float about the centroid; here double sums relative to p0.
 * rsreg_cloud_plane_count: the scoring stage alone.  counts_out[h] = the inliers of coeffs[4 h .. 4 h + 3] (host), h < H.  H == 0:
 *   nothing is written.  n == 0: zeros.
 * rsreg_cloud_plane_hypotheses: the sampler and the fit alone, for the hypotheses h_first .. h_first + H - 1 (every output host memory
 *   and nullable).  coeffs_out[4 j ..]: the model, quiet NaN x 4 for an invalid hypothesis; samples_out[4 j ..]: i0, i1, i2 and the
 *   good try (-1 x 4 after sixteen bad tries; a hypothesis that fails the axis test alone keeps its sample); valid_out[j]: 1 or 0.
 * rsreg_cloud_plane_segment: SACSegmentation::segment.  params NULL: rsreg_plane_params_default.  coeff_out[4]: the model (refined
 *   if `refined`).  indices_out: the inliers' record indices, ascending; *n_inliers_out their number -- when it exceeds `capacity`
 *   the first `capacity` are written and the call still returns RSREG_OK.  coeff_out, indices_out (with capacity 0), n_inliers_out
 *   and result may be NULL.
 * rsreg_cloud_plane_filter: keeps the inliers of one model -- negative: every other record, the ones that are not finite included.
 *   out, in == out, keep_organized, is_dense, the versioning and *n_kept are those of rsreg_cloud_radius_outlier_removal, through
 *   the same flag / scan / gather kernels.
 * rsreg_cloud_extract_indices: pcl::ExtractIndices over a HOST list of n_indices int32.  Positive: out record j = in record
 *   indices[j], order and repeats as given (width = n_indices, height 1).  Negative: the records not named, in input order.  An
 *   index outside the cloud: RSREG_ERR_INVALID_ARG, checked on the host before anything is launched.  in == out is allowed.
 * Every output is a function of the cloud and the parameters alone, the same bytes from any context: the counts are integers, the
 *   generator is a function of (seed, h, draw), every float sum has its order written above.
 * Not built: the other models (line, sphere, cylinder, normal plane), SAC_LMEDS / MSAC and kin, setSamplesMaxDist, setIndices on the
 *   segmentation, PCL's refineModel, segmentation across ranks (every rank segments the cloud it holds). */
#define RSREG_NUM_PLANE_SEG_SUMS 10
typedef struct rsreg_plane_params {
    double distance_threshold;     /* setDistanceThreshold; 0: the caller sets it */
    double probability;            /* 0.99 */
    double axis[3];                /* setAxis; {0, 0, 0}: no constraint */
    double eps_angle;              /* setEpsAngle, radians; 0: no constraint */
    int32_t max_iterations;        /* 50 (SACSegmentation's default) */
    int32_t optimize_coefficients; /* 1 */
    uint64_t seed;                 /* 0 */
} rsreg_plane_params;
typedef struct rsreg_plane_result {
    int32_t found;
    int32_t best_hypothesis;
    int32_t sample[3];             /* the winner's three records */
    int32_t iterations;            /* valid hypotheses the replay consumed */
    int32_t skipped;               /* invalid hypotheses the replay consumed */
    int32_t refined;               /* 1: coeff_out is the refined model; 0: the winner's own */
    uint64_t n_inliers;
    double cos_eps;                /* std::cos(eps_angle) as used; 0 when the constraint does not apply */
    float unrefined[4];            /* the winner's own model */
    double sums[RSREG_NUM_PLANE_SEG_SUMS];   /* the refinement's sums; zeros when there was none */
} rsreg_plane_result;
void rsreg_plane_params_default(rsreg_plane_params *p);
int rsreg_plane_from_sums(const double sums[RSREG_NUM_PLANE_SEG_SUMS], const float p0[3], const float prior[4], float coeff_out[4]);
int rsreg_cloud_plane_count(rsreg_ctx *ctx, const rsreg_cloud *in, const float *coeffs /* H*4 */, size_t H, double threshold,
                            uint32_t *counts_out /* H */);
int rsreg_cloud_plane_hypotheses(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_plane_params *params, uint64_t h_first, size_t H,
                                 float *coeffs_out /* H*4 */, int32_t *samples_out /* H*4 */, int32_t *valid_out /* H */);
int rsreg_cloud_plane_segment(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_plane_params *params /* may be NULL */, float coeff_out[4],
                              int32_t *indices_out, size_t capacity, size_t *n_inliers_out, rsreg_plane_result *result /* may be NULL */);
int rsreg_cloud_plane_filter(rsreg_ctx *ctx, const rsreg_cloud *in, const float coeff[4], double threshold, int negative, int keep_organized,
                             rsreg_cloud *out, uint64_t *n_kept /* may be NULL */);
int rsreg_cloud_extract_indices(rsreg_ctx *ctx, const rsreg_cloud *in, const int32_t *indices, size_t n_indices, int negative, rsreg_cloud *out,
                                uint64_t *n_kept /* may be NULL */);
/* ---- pcl::FPFHEstimationOMP with setRadiusSearch(radius): SPFH and FPFH over the radius search above -- a support of fixed
 * metric size, any number of neighbours.  PCL 1.9.1 features/impl/fpfh.hpp (computePointSPFHSignature, weightPointSPFHSignature)
 * and pfh_tools.cpp (computePairFeatures), recalled; PCL is not available to check against, so what follows IS the contract.
 * normals: as for rsreg_cloud_fpfh (n records of the same context, three floats first, stride >= 12 and a multiple of 4).
 * Neighbourhood N_r(i): exactly the radius search's -- the finite records j with float32 d2(i, j) < (float)((double)radius *
 * (double)radius), strictly; the record itself and exact copies among them; no cap.  m(i) = their number = what
 * rsreg_cloud_radius_count gives.
 * Pair features and bins: those of rsreg_cloud_fpfh above, unchanged (double, no contraction).  A pair is skipped when j == i,
 * when f4 == 0 (exact copies), when |v| == 0, or when n_i or n_j is not finite.
 * SPFH row of record i: a bin hit by c pairs holds the float that adding hist_incr = 100.0f / (float)(m - 1) to 0.0f c times
 * gives (PCL's sequential +=), for any c up to m - 1.  m == 1: no pair, no addition, a row of zeros -- the infinite increment is
 * never used.  A record that is not finite, or whose own normal is not finite, has an all-zero row (and is a neighbour of others
 * with that row).
 * FPFH row of record i.  The weights and the products are PCL's float32:
 *   for every j in N_r(i) with d2(i, j) != 0:  w = 1.0f / d2;  val[b] = SPFH[j][b] * w  (float32, no contraction);
 *     H[b] += (double)val[b]
 *   S_t = ((H[11t] + H[11t + 1]) + ...) + H[11t + 10] in double;  out[b] = (float)(H[b] * (S_t != 0 ? 100.0 / S_t : 0.0)).
 * Both quirks of PCL are kept: the weight is 1 / SQUARED distance, and the record's own SPFH does not enter.  A record with no
 * neighbour at positive distance gives 33 zeros.  A record that is not finite, or whose own normal is not finite, gets 33 quiet
 * NaNs.  NaNs the arithmetic makes (a denormal d2 gives w = +inf, and 0 * inf is NaN) stand where it puts them, sign and payload
 * not specified.  is_dense is 0 if any row holds a NaN, otherwise the input's.
 * DEVIATION FROM PCL 1.9.1, stated: H is accumulated in DOUBLE, in an order that is a function of the cloud and the radius alone
 * (inside a cell of the index the points lie in ascending record index) -- the deviation rsreg_cloud_normals_radius makes.  PCL
 * adds the float products in float in FLANN's distance-sorted order; that is not reproduced: it would need a per-record sort of a
 * list without a bound, and FLANN leaves the order of equal distances open anyway.  A PCL build agrees to float rounding of the
 * sums (and to the pair features' deviation stated above).
 * radius not finite or <= 0, normals of another size or context, out == in, out == normals, a null argument:
 * RSREG_ERR_INVALID_ARG, nothing launched, `out` untouched.  An empty cloud gives an empty cloud of 132-byte records; a cloud
 * without a finite record gives NaN rows, zero SPFH rows and zero counts.  The same cloud, normals and radius give the same bytes
 * whatever the context has indexed before.  Every call builds its index and walks it twice; no neighbour list is stored.
 * Not built: setIndices, other bin counts, PFH.  setSearchSurface: rsreg_cloud_fpfh_radius_surface, below.
 *
 * rsreg_cloud_fpfh_radius: out = n records of 132 bytes laid out as pcl::FPFHSignature33, width and height as the input's.  Waits
 * for the stream (whether a row holds a NaN).
 * rsreg_cloud_spfh_radius: host_out = the n * 33 floats of the SPFH rows, count_out[i] = m(i) (0 for a non-finite record), the
 * caller's record order. */
int rsreg_cloud_fpfh_radius(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, double radius, rsreg_cloud *out);
int rsreg_cloud_spfh_radius(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_cloud *normals, double radius, float *host_out /* n*33 */,
                            uint32_t *count_out /* n, may be NULL */);
/* ---- setSearchSurface with setRadiusSearch(radius): the records of one cloud (the QUERIES: PCL's setInputCloud, nq of them) are
 * searched for in another (the SURFACE: PCL's setSearchSurface, ns records), as PCL users compute normals and descriptors AT
 * keypoints OVER the dense frame.  PCL 1.9.1 features/impl/feature.hpp (initCompute, searchForNeighbors) and fpfh.hpp
 * (computeSPFHSignatures, computeFeature), recalled; PCL is not available to check against, so what follows IS the contract.
 * Every cloud is a cloud of the context with records as above (x, y, z floats first, stride >= 12 and a multiple of 4); queries
 * and surface may be the same handle.
 * Neighbourhood: surface record j is a neighbour of finite query record i when j is finite and float32 d2(i, j) < (float)((double)
 * radius * (double)radius), strictly -- the rule above, unchanged.  A query is not a neighbour of anything; a surface record that
 * coincides with the query counts like any other.  m(i) = their number; it may be 0; a non-finite query has m = 0.
 * Order: every sum runs in the order of the index over the SURFACE -- a function of the surface and the radius alone, not of the
 * queries, their order, or what the context indexed before.  With queries == surface the counts and the normals are therefore the
 * bytes of rsreg_cloud_radius_count and rsreg_cloud_normals_radius, and the FPFH rows are the bytes of rsreg_cloud_fpfh_radius on
 * every record whose own normal is finite (the in-cloud call's NaN rule for a record's own normal does not exist here: the query has
 * no normal and none is looked at).
 * radius not finite or <= 0, normals whose size is not the surface's, a cloud of another context, `out` equal to an input, a null
 * argument: RSREG_ERR_INVALID_ARG, nothing launched, `out` untouched.  Empty queries give an empty `out` of the right stride; an
 * empty surface, or one without a finite record, gives every count 0, every row NaN and *n_spfh = 0.  Every call builds its own
 * index over the surface.  Not built: setKSearch with a search surface (the k nearest samples of a dense surface are a support of
 * a few millimetres), setIndices, neighbour lists as an output, PFH.
 *
 * rsreg_cloud_radius_count_surface: host_out[i] = m(i), nq uint32 in the queries' record order.
 * rsreg_cloud_normals_radius_surface: the covariance of rsreg_cloud_normals_radius, unchanged -- C from d = neighbour - query
 * record in double over the m surface neighbours; eigenvector, curvature, the flip (towards the viewpoint FROM THE QUERY RECORD)
 * and the trace-0 case as they are.  m < 3 or a non-finite query: four quiet NaNs.  out: nq pcl::Normal records, width and height
 * the queries'; is_dense 0 if any row got NaNs, otherwise the queries' own.  Waits for the stream.
 * rsreg_cloud_fpfh_radius_surface, rsreg_cloud_spfh_radius_surface: surface_normals holds one record per surface record.
 *   The SPFH row of a surface record is EXACTLY the row rsreg_cloud_spfh_radius(surface, surface_normals, radius) gives it: its
 *   neighbourhood in the surface, the surface's normals, the same bytes.  A row is computed only for the surface records that are
 *   a neighbour of at least one finite query (PCL's spfh_indices set): *n_spfh is the size of that set, needed_out[j] is 1 or 0,
 *   and a host_out row that is not needed is zero.
 *   The FPFH row of query i is the weighting above over its surface neighbours j with d2(i, j) != 0: w = 1.0f / d2 and
 *   SPFH[j][b] * w in float32, H in double in the order of the surface's index, the block sums and the scaling as they are.
 *   33 quiet NaNs for a non-finite query AND FOR A QUERY WITH m = 0 (PCL's searchForNeighbors(...) == 0 branch, recalled); 33
 *   zeros when m > 0 but every neighbour is at distance 0.  out: nq records of 132 bytes, width and height the queries'; is_dense
 *   0 if any row holds a NaN, otherwise the queries' own.  Both wait for the stream (the number of needed records).
 *   count_out[i] = m(i) in the queries' record order. */
int rsreg_cloud_radius_count_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface, double radius,
                                     uint32_t *host_out /* nq */);
int rsreg_cloud_normals_radius_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface, double radius,
                                       const float viewpoint[3], rsreg_cloud *out);
int rsreg_cloud_fpfh_radius_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface,
                                    const rsreg_cloud *surface_normals, double radius, rsreg_cloud *out, uint64_t *n_spfh /* may be NULL */);
int rsreg_cloud_spfh_radius_surface(rsreg_ctx *ctx, const rsreg_cloud *queries, const rsreg_cloud *surface,
                                    const rsreg_cloud *surface_normals, double radius, float *host_out /* ns*33 */,
                                    uint32_t *needed_out /* ns, may be NULL */, uint32_t *count_out /* nq, may be NULL */);
/* pcl::IntegralImageNormalEstimation on an ORGANIZED cloud of w x h records P[r][c] (src/edge_extractor.hpp:9-15 runs it with
 * AVERAGE_3D_GRADIENT, setMaxDepthChangeFactor(0.02f), setNormalSmoothingSize(10.0f) on every frame): a cost per pixel that
 * does not depend on the scene, and no index.  PCL 1.9.1 features/impl/integral_image_normal.hpp, recalled; PCL is not
 * available to check against, so what follows IS the contract.  f = max_depth_change_factor, s = normal_smoothing_size,
 * B = (int)s, z = P.z; (a) - (d) are float32.
 * (a) depth changes: M = 1 everywhere; for r in [0, h-1), c in [0, w-1): t = (f * (fabsf(z[r][c]) + 1.0f)) * 2.0f; if
 *     fabsf(z[r][c] - z[r][c+1]) > t, or either depth is not finite, M[r][c] = M[r][c+1] = 0; likewise with z[r+1][c].
 * (b) distance map: D[i] = 0 where M == 0, else (float)(w + h), i = r * w + c, then two sequential chamfer passes,
 *     forward:  r = 1 .. h-1, c = 1 .. w-1:  m = min(min(D[i-w-1] + 1.4f, D[i-w] + 1.0f), min(D[i-1] + 1.0f, D[i-w+1] + 1.4f)),
 *     backward: r = h-2 .. 0, c = w-2 .. 0:  m = min(min(D[i+w-1] + 1.4f, D[i+1] + 1.0f), min(D[i+w] + 1.0f, D[i+w+1] + 1.4f)),
 *     each followed by  if (m < D[i]) D[i] = m.  The flat indices are PCL's: the forward pass never writes column 0 and at
 *     c = w-1 reads D[r][0] as its "up-right"; the backward pass never writes column w-1 or row h-1 and at c = 0 reads
 *     D[r][w-1] as its "lower-left".
 * (c) window: for r in [B, h-B), c in [B, w-B) with finite z: sm = min(D[r][c], s); if sm > 2.0f the window size is
 *     R = (int)sm, else the record has no normal; neither has anything in the B-wide border (w <= 2B or h <= 2B: no record
 *     has a normal; not an error).
 * (d) differences: DX[r][c] = P[r][c+1] - P[r][c-1], DY[r][c] = P[r+1][c] - P[r-1][c] per component for 1 <= r < h-1,
 *     1 <= c < w-1, zero elsewhere; an element is finite when the float sum (x + y) + z is.
 * (e) normal: over columns [c - R/2, c - R/2 + R) and rows [r - R/2, r - R/2 + R) (integer division: not centred for even R)
 *     gx = the double sum of the finite DX elements, gy of the finite DY elements; none of either: no normal.
 *     n = gy x gx in double, every product and difference one IEEE operation; l = (n0^2 + n1^2) + n2^2; l == 0: no normal;
 *     n_i / sqrt(l), each rounded to float; flipped as rsreg_cloud_normals flips: with v = viewpoint - P in float, when
 *     (v.x * nx + v.y * ny) + v.z * nz < 0.
 * out (!= in): w x h records of 32 bytes laid out as pcl::Normal, width and height the input's, is_dense = 0 always.  A record
 * without a normal: four quiet NaNs (normal and curvature), the other words 0.  A record with one: curvature = quiet NaN
 * (this method defines none).  rect_out (nullable, host, w * h bytes): R of every record, 0 = no window -- (a) - (c) on
 * their own; waits for the stream.  The same cloud gives the same bytes whatever the context ran before.
 * RSREG_ERR_INVALID_ARG, out untouched: an unorganized cloud (height == 1), any method but AVERAGE_3D_GRADIENT,
 * depth_dependent_smoothing, a border policy other than IGNORE, s outside (0, 64], f negative or not finite, a frame wider
 * than 8192 pixels.
 * DEVIATION FROM PCL 1.9.1, stated: PCL takes the window sums from a summed-area table filled by
 * S[r][c] = S[r-1][c] + S[r][c-1] - S[r-1][c-1] + x in double; here gx, gy are the double sums of the window's elements
 * themselves, row by row.  Where every coordinate is a multiple of 2^-12 below 16 all such sums are exact and the two
 * agree in every bit; elsewhere they differ by the rounding of PCL's table, about 1e-11 of a sum. */
enum rsreg_iin_method {   /* pcl::IntegralImageNormalEstimation::NormalEstimationMethod */
    RSREG_IIN_COVARIANCE_MATRIX = 0, RSREG_IIN_AVERAGE_3D_GRADIENT = 1, RSREG_IIN_AVERAGE_DEPTH_CHANGE = 2, RSREG_IIN_SIMPLE_3D_GRADIENT = 3
};
enum rsreg_iin_border_policy { RSREG_IIN_BORDER_IGNORE = 0, RSREG_IIN_BORDER_MIRROR = 1 };   /* ...::BorderPolicy */
typedef struct rsreg_iin_params {
    int method;                       /* rsreg_iin_method */
    float max_depth_change_factor, normal_smoothing_size;
    int depth_dependent_smoothing, border_policy;
    float viewpoint[3];
} rsreg_iin_params;
/* PCL's defaults: AVERAGE_3D_GRADIENT, 0.02f, 10.0f, no depth-dependent smoothing, IGNORE, viewpoint (0, 0, 0) */
void rsreg_iin_params_default(rsreg_iin_params *params);
int rsreg_cloud_integral_normals(rsreg_ctx *ctx, const rsreg_cloud *in, const rsreg_iin_params *params /* NULL = defaults */,
                                 rsreg_cloud *out, uint8_t *rect_out /* may be NULL */);
/* ---- capture: a depth frame and a colour frame -> an organized PointXYZRGB cloud -----------------------------------------
 * The step in front of everything above.  The reference makes the vertices and texture coordinates with rs2::pointcloud
 * (map_to, calculate) and the records with convert_to_pcl (src/capture.hpp:72-107: the three-fifths centre crop that
 * blur_filter.hpp repeats) or convert_to_pcl_new (src/capture_opencv.hpp:128-160: the whole frame), the colour through
 * rgb_texture (src/capture.hpp:11-32).  Here the two images go in -- 5 bytes a pixel instead of the 32 of a record -- and the
 * cloud is built in HBM.  librealsense is not available to check against: what follows is RECALLED from librealsense 2.3x
 * (include/librealsense2/rsutil.h: rs2_deproject_pixel_to_point, rs2_transform_point_to_point, rs2_project_point_to_pixel;
 * src/proc/pointcloud.cpp) and IS the contract.  All arithmetic is float32; every operation written below is one IEEE
 * operation rounded once, in the order written (C's left-to-right parse), none contracted into a multiply-add.
 *
 * Images.  depth: p->depth.height rows of p->depth.width uint16 values, `depth_stride` bytes apart (even, >= 2 * width).
 * colour: p->color.height rows of p->color.width pixels of p->color_bytes_per_pixel (3 or 4) bytes, `color_stride` bytes
 * apart (>= bytes per pixel * width).  The two images need not have the same size.
 * (1) Vertex of depth pixel (c, r) with raw value d:
 *       depth = depth_scale * (float)d;   x = ((float)c - ppx) / fx;   y = ((float)r - ppy) / fy      (depth intrinsics)
 *     and, when the depth model is RSREG_DISTORTION_INVERSE_BROWN_CONRADY (k = depth.coeffs):
 *       r2 = x*x + y*y;   f = 1 + k[0]*r2 + k[1]*r2*r2 + k[4]*r2*r2*r2;
 *       ux = x*f + 2*k[2]*x*y + k[3]*(r2 + 2*x*x);   uy = y*f + 2*k[3]*x*y + k[2]*(r2 + 2*y*y);   x = ux;  y = uy;
 *     P = (depth * x, depth * y, depth).  For d = 0 these are the computed products: -0 where x or y is negative.
 * (2) Texture coordinate: if P.z == 0 then (u, v) = (0, 0).  Otherwise, with R = rotation (column-major), t = translation:
 *       q[k] = R[0+k]*P.x + R[3+k]*P.y + R[6+k]*P.z + t[k]    (k = 0, 1, 2; added left to right)
 *       x = q[0] / q[2];   y = q[1] / q[2]
 *     and, when the colour model is RSREG_DISTORTION_MODIFIED_BROWN_CONRADY (k = color.coeffs):
 *       r2 = x*x + y*y;   f = 1 + k[0]*r2 + k[1]*r2*r2 + k[4]*r2*r2*r2;   x = x*f;   y = y*f;
 *       dx = x + 2*k[2]*x*y + k[3]*(r2 + 2*x*x);   dy = y + 2*k[3]*x*y + k[2]*(r2 + 2*y*y);   x = dx;  y = dy;
 *     (librealsense's form: dx, dy take the scaled x, y and the r2 from before the scaling), then with the colour intrinsics
 *       px = x*fx + ppx;   py = y*fy + ppy;   u = px / (float)width;   v = py / (float)height
 *     There is no half-pixel term here: the + .5f of (3) is the rounding.
 * (3) Colour (rgb_texture): xi = min(max(I(u * (float)width + .5f), 0), width - 1), yi likewise from v and the height, where
 *     I(t) is C's (int)t: truncation toward zero, and for a t that is NaN or outside [-2^31, 2^31) -- undefined in C -- INT_MIN,
 *     what the x86 conversion the reference ran on gives, so that xi = 0.  (A GPU's conversion saturates: +inf would land on
 *     width - 1.  The rule is written out in the code, not left to the instruction.)  The three bytes at
 *     yi * color_stride + xi * bytes_per_pixel are, with color_bgr = 1 (the reference: "BGR due to Camera Model"),
 *     b, g, r in that order; with color_bgr = 0, r, g, b.  A fourth byte is skipped.
 * (4) Records: the window rows [r0, r1) x cols [c0, c1) of the depth image, row-major, goes to records 0, 1, 2 ... LINEARLY (the
 *     reference's i++), not by output row: x, y, z, 1.0f, rgba = 0xff000000 | r << 16 | g << 8 | b, three zero words.  The
 *     cloud has out_width * out_height records; those past the window's count stay the default PointXYZRGB
 *     (0, 0, 0, 1, 0xff000000).  width = out_width, height = out_height, is_dense as given.
 * Distortion models: none, inverse Brown-Conrady on the depth side, modified Brown-Conrady on the colour side.  Any other
 * pairing (a model value of 0 .. 5) is accepted only when all five coefficients are zero and then acts as none (the D435i
 * reports Brown-Conrady with zero coefficients); with a non-zero coefficient, or a model outside 0 .. 5: RSREG_ERR_INVALID_ARG.
 * RSREG_DISTORTION_NONE ignores its coefficients.
 * RSREG_ERR_INVALID_ARG as well, nothing written: a zero image size or output size; a window outside the depth image
 * (0 <= r0 <= r1 <= height, 0 <= c0 <= c1 <= width must hold; an empty window is allowed: all records default);
 * (r1 - r0) * (c1 - c0) > out_width * out_height; more than 2^31 - 16 records; bytes per pixel other than 3 or 4; a stride
 * smaller than a row, or an odd depth stride.
 * OUT OF SCOPE, not built: an asynchronous or deferred variant through the upload worker; the iterative (forward)
 * Brown-Conrady, F-Theta and Kannala-Brandt models with non-zero coefficients; the infrared fallback, alignment of depth to
 * colour as an image, and IMU handling of the reference's capture loop; the SIFT code of capture_opencv.hpp. */
enum rsreg_distortion {   /* rs2_distortion, same values */
    RSREG_DISTORTION_NONE = 0, RSREG_DISTORTION_MODIFIED_BROWN_CONRADY = 1, RSREG_DISTORTION_INVERSE_BROWN_CONRADY = 2,
    RSREG_DISTORTION_FTHETA = 3, RSREG_DISTORTION_BROWN_CONRADY = 4, RSREG_DISTORTION_KANNALA_BRANDT4 = 5
};
typedef struct rsreg_intrinsics {   /* rs2_intrinsics, same order: 48 bytes */
    int32_t width, height;
    float ppx, ppy, fx, fy;
    int32_t model;                  /* rsreg_distortion */
    float coeffs[5];
} rsreg_intrinsics;
typedef struct rsreg_depth_params {   /* 192 bytes */
    rsreg_intrinsics depth, color;
    float rotation[9], translation[3];   /* rs2_extrinsics depth -> colour: column-major 3 x 3, metres */
    float depth_scale;                   /* metres per depth unit (rs2::depth_sensor::get_depth_scale; D400: 0.001) */
    int32_t color_bytes_per_pixel;       /* 3 or 4 */
    int32_t color_bgr;                   /* 1: bytes b, g, r (the reference); 0: bytes r, g, b */
    int32_t r0, r1, c0, c1;              /* the window over the depth image: rows [r0, r1), cols [c0, c1) */
    uint32_t out_width, out_height;      /* the cloud's shape: out_width * out_height records */
    int32_t is_dense;
    uint32_t reserved[2];                /* 0 */
} rsreg_depth_params;
/* convert_to_pcl_new: the whole w x h depth frame, the cloud w x h, is_dense = 0.  Everything else is a placeholder for the
 * caller to overwrite from the camera: both intrinsics w x h with ppx = w / 2, ppy = h / 2, fx = fy = w and no distortion,
 * identity extrinsics, depth_scale 0.001, 3 bytes per pixel, color_bgr = 1. */
void rsreg_depth_params_default(uint32_t w, uint32_t h, rsreg_depth_params *p);
/* convert_to_pcl / BlurFilter, C integer division: rows [h/5, h/5*4), cols [w/5, w/5*4), out_width = w*3/5,
 * out_height = h*3/5, is_dense = 1 (PCL's default, which the reference leaves untouched); the rest as above.  Window and
 * shape disagree for many sizes -- w = 848: 507 columns are written into a cloud 508 wide -- which is the reference's
 * behaviour and is kept: the fill is linear, the tail stays default. */
void rsreg_depth_params_reference(uint32_t w, uint32_t h, rsreg_depth_params *p);
/* The contract restated sequentially on the host (no context needed): host images in, out_width * out_height 32-byte records
 * out (capacity_records must hold them); *width, *height, *is_dense (each nullable) receive the cloud's. */
int rsreg_depth_to_cloud(const void *depth, size_t depth_stride, const void *color, size_t color_stride,
                         const rsreg_depth_params *p, void *out, size_t capacity_records, uint32_t *width, uint32_t *height,
                         int *is_dense);
/* The same on the GPU, the same bytes (csrc/depthcloud.hip: one lane per record, two 16-byte stores).  Host images: the
 * two images are staged and go over the link, not the records; both have been read when the call returns.  On the context's
 * stream; `out` follows the versioning rules (its version changes). */
int rsreg_cloud_from_depth(rsreg_ctx *ctx, const void *depth, size_t depth_stride, const void *color, size_t color_stride,
                           const rsreg_depth_params *p, rsreg_cloud *out);
/* ... with the two images already in HBM (d_depth 2-byte aligned): nothing crosses the link.  The images must stay alive and
 * unchanged until the next synchronising call on the context has returned. */
int rsreg_cloud_from_depth_device(rsreg_ctx *ctx, const void *d_depth, size_t depth_stride, const void *d_color,
                                  size_t color_stride, const rsreg_depth_params *p, rsreg_cloud *out);
/* icp.setInputTarget / setInputSource / align on handles; aligned_out (nullable, may be the source
 * cloud): the source records with xyz <- final * xyz and data[3] = 1 */
int rsreg_icp_set_target_cloud(rsreg_ctx *ctx, const rsreg_cloud *cloud, double max_correspondence_distance);
int rsreg_icp_set_source_cloud(rsreg_ctx *ctx, const rsreg_cloud *cloud);
/* 1 when the ICP target index of `ctx` was built by rsreg_icp_set_target_cloud from this cloud, whose records have not
 * been rewritten since, for this gate; 0 otherwise.  The ICP edge scheme sets the same grown feature cloud as the target
 * of its coarse and of its refining ICP, one after the other (icp_edge_based_registration.hpp:94-95,108-109): a caller
 * that asks first may skip the second build (pcl_compat.hpp: setReuseTargetIndex). */
int rsreg_icp_target_is_cloud(const rsreg_ctx *ctx, const rsreg_cloud *cloud, double max_correspondence_distance);
int rsreg_icp_align_cloud(rsreg_ctx *ctx, const float *guess, const rsreg_icp_params *params,
                          rsreg_icp_result *result, rsreg_cloud *aligned_out);
/* ndt.setInputTarget / align on handles, and on raw device pointers */
int rsreg_ndt_set_target_cloud(rsreg_ctx *ctx, const rsreg_cloud *cloud, double resolution);
int rsreg_ndt_align_cloud(rsreg_ctx *ctx, const rsreg_cloud *source, const float *guess,
                          const rsreg_ndt_params *params, rsreg_ndt_result *result, rsreg_cloud *aligned_out);
int rsreg_ndt_set_target_device(rsreg_ctx *ctx, const void *d_points, size_t n, size_t stride, int is_dense,
                                double resolution);
int rsreg_ndt_align_device(rsreg_ctx *ctx, const void *d_source, size_t n, size_t stride, int is_dense,
                           const float *guess, const rsreg_ndt_params *params, rsreg_ndt_result *result,
                           void *d_aligned_out);
/* Registration::getFitnessScore(max_range) of the last rsreg_ndt_align / _align_device / _align_cloud, as
 * rsreg_icp_fitness_score: PCL scores NDT against a kd-tree over the target's POINTS (not its voxels), which
 * rsreg_ndt_set_target* keeps for this.  The same squared-range quirk; DBL_MAX when nothing is in range; RSREG_ERR_STATE before
 * an alignment against the current NDT target. */
int rsreg_ndt_fitness_score(rsreg_ctx *ctx, double max_range, double *score, uint64_t *n_within);

/* ---- edge features: extract_edge_features (src/edge_extractor.hpp:7-39) -------------------- */
/* The reference's TwoPhaseRegistrationScheme::extract_features (icp_edge...hpp:21-23, ndt_edge...hpp:18-20).
 * Of everything that function computes it returns only the points labelled EDGELABEL_RGB_CANNY
 * (label_indices[4]): pcl::Edge::detectEdgeCanny (thresholds 40 / 100) on the gray image
 * float((r + g + b) / 3) of the ORGANIZED cloud (width x height records, rgb at byte 16).  out must
 * hold width*height records; indices_out (nullable) receives the edge points' indices, ascending. */
int rsreg_extract_edge_features(rsreg_ctx *ctx, const void *points, uint32_t width, uint32_t height, size_t stride,
                                void *out, int32_t *indices_out, size_t *n_out);
int rsreg_cloud_edge_features(rsreg_ctx *ctx, const rsreg_cloud *in, rsreg_cloud *out);
/* rsreg_cloud_edge_features queued like rsreg_cloud_filter_async: the edge schemes extract (and then filter) the features
 * of frame k + 1 beside the two alignments of frame k -- the reference extracts the features of all frames before it
 * registers any (types.hpp:30-43).  `in` may still be uploading (rsreg_cloud_upload_deferred): the job waits for it, not
 * the caller.  Same lifetime rule as above. */
int rsreg_cloud_edge_features_async(rsreg_ctx *ctx, const rsreg_cloud *in, rsreg_cloud *out);

/* ---- PCD files: the LZF coder of "DATA binary_compressed" bodies (host only, no ctx) ------ */
/* pcl::io::loadPCDFile / savePCDFileBinaryCompressed as reached from main.cpp:53,81,87: the body
 * is u32 compressed size, u32 uncompressed size, then one LZF stream over the fields laid out one
 * after the other.  encode/decode return the number of bytes written, 0 on failure (capacity
 * too small, malformed stream). */
size_t rsreg_lzf_max_encoded_size(size_t n);
size_t rsreg_lzf_encode(const void *in, size_t n, void *out, size_t capacity);
size_t rsreg_lzf_decode(const void *in, size_t n, void *out, size_t capacity);

/* ---- introspection (tests, bench) --------------------------------------------------- */
typedef struct rsreg_grid_info {
    float origin[3];
    float cell_size;
    int32_t dims[3];
    uint32_t n_target_points;   /* finite points handed in                                  */
    uint32_t n_unique_points;   /* after dropping exact duplicates (same xyz bits)          */
    uint32_t n_cells;           /* occupied cells                                           */
    uint32_t max_points_per_cell;
    double ms_build;            /* device time of the last build (profiling on)             */
    uint32_t index_kind;        /* 1 = dense cell-start table, 0 = brick hash (huge extents), 2 = none: a device-cloud
                                 * target set for at most 64 source points is searched whole (IncrementalICP) */
    uint32_t n_source_distinct; /* distinct source points the iterations work on (0: no source) */
    uint64_t index_bytes;       /* HBM bytes of the index: sorted points + tables           */
} rsreg_grid_info;
/* (waits for an index build that rsreg_icp_set_target* has queued and not waited for: the two counts come with it) */
int rsreg_icp_grid_info(rsreg_ctx *ctx, rsreg_grid_info *info);

/* Where the HOST-pointer entry points (rsreg_icp_set_source, rsreg_icp_set_target, rsreg_icp_align with aligned_out: the
 * literal call surface of incremental_icp.hpp:57-63, clouds in host memory in, 4x4 and aligned cloud out) spent the host's
 * wall clock in their last call, ms.  *_stage_wait: waiting for the staging buffer's previous trip over the link;
 * *_pack: packing the caller's records into pinned memory and queueing their copies (the copies run meanwhile);
 * target_build: the index build, behind the target's copy (ends with the host's wait for the build's counts);
 * align: rsreg_icp_begin .. the last iteration; aligned_copy: the aligned cloud's way home, device -> pinned -> caller. */
typedef struct rsreg_host_timing {
    double source_stage_wait, source_pack, target_stage_wait, target_pack, target_build, align, aligned_copy;
    double loop_enqueue;   /* device-resident loop: what queueing all its launches took the calling thread (0.4: was `reserved`) */
} rsreg_host_timing;
int rsreg_ctx_host_timing(rsreg_ctx *ctx, rsreg_host_timing *out);

#ifdef __cplusplus
}
#endif
#endif /* RSREG_H_ */
