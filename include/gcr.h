/*
 * gcr.h -- C ABI of the MI355X-native Graph-Cut RANSAC rectification engine.
 *
 * This is the drop-in boundary for the reference's hot path.  Each entry point
 * replaces one C++ function that pygcransac's pybind11 layer binds today
 * (yuvalnis/graph-cut-ransac, src/pygcransac/include/gcransac_python.h):
 *
 *   gcr_rect_scale_only(..., original=0)  <- findRectifyingHomographyScaleOnly_
 *                                            (gcransac_python.h:7-18, .cpp:32-142)
 *   gcr_rect_scale_only(..., original=1)  <- findRectifyingHomographyScaleOnlyOriginal_
 *                                            (gcransac_python.h:20-31, .cpp:144-254)
 *   gcr_rect_sift(...)                    <- findRectifyingHomographySIFT_
 *                                            (gcransac_python.h:33-47, .cpp:256-406)
 *
 * Conventions (no C++ or torch types cross this boundary):
 *   - features are row-major N x 3 float64 arrays, exactly the flat buffers the
 *     reference copies out of numpy (bindings.cpp:12-17, 234-250);
 *   - the caller owns every buffer; masks are N bytes (0/1);
 *   - H_out is the row-major 3x3 homography model.getHomography() / H22
 *     (gcransac_python.cpp:95-104);
 *   - return value >= 0 is the total number of inliers (the reference's int
 *     return, gcransac_python.cpp:141/405), < 0 is an error code; the message is
 *     available from gcr_last_error() (thread-local).  -EINVAL maps to Python
 *     ValueError, everything else to RuntimeError.
 *   - no exceptions cross the ABI; functions are thread-safe for distinct
 *     contexts; one context per device.
 */
#ifndef GCR_H_
#define GCR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Guided sampling (gcr_problem_set_probabilities, the *_guided entries and
 * their debug hooks) was added without a version change: every addition is a
 * new function, no struct changed size or layout, so the version stays 5.
 * The same holds for the guided stop: GCR_FLAG_GUIDED_STOP is a new bit of
 * gcr_params.flags (a call that leaves it clear runs as before), its host
 * and debug entries are new functions.  The essential-matrix estimator
 * (GCR_SOLVER_ESSENTIAL5) likewise: new functions and a new solver kind only;
 * and so the one with known gravity (GCR_SOLVER_ESSENTIAL3_GRAVITY), the
 * host hook gcr_host_guided_index, and the homography from two SIFT
 * correspondences (GCR_SOLVER_HOMOGRAPHY2_SIFT).  PROSAC sampling and its
 * stop (GCR_FLAG_PROSAC_STOP) likewise: a new flag bit and new functions.
 * NAPSAC sampling (gcr_problem_set_napsac and its host hooks): new functions
 * only.  gcr_verify_many and its host twin: two new functions and their own
 * result struct. */
#define GCR_ABI_VERSION 5

/* error codes */
#define GCR_OK 0
#define GCR_EINTERNAL (-1)
#define GCR_EHIP (-5)
#define GCR_ENOMEM (-12)
#define GCR_ENODEV (-19)
#define GCR_EINVAL (-22)

/* solver kinds (types.h:43-59 estimator typedefs) */
#define GCR_SOLVER_SCALE3 0          /* RectifyingHomographyThreeSIFTSolver         */
#define GCR_SOLVER_SCALE3_ORIGINAL 1 /* RectifyingHomographyThreeSIFTSolverOriginal */
#define GCR_SOLVER_SIFT22 2          /* RectifyingHomographyTwoSIFTSolver           */
#define GCR_SOLVER_HOMOGRAPHY4 3     /* 4-point homography (upstream GC-RANSAC)     */
#define GCR_SOLVER_FUNDAMENTAL7 4    /* 7-point fundamental matrix (upstream)       */
#define GCR_SOLVER_ESSENTIAL5 5      /* 5-point essential matrix (upstream); problems of
                                        this kind come from gcr_problem_create_essential */
#define GCR_SOLVER_ESSENTIAL3_GRAVITY 6 /* 3-point essential matrix with the gravity direction
                                        of both cameras known; problems of this kind come
                                        from gcr_problem_create_gravity_essential */
#define GCR_SOLVER_HOMOGRAPHY2_SIFT 7 /* homography from two SIFT correspondences (point, feature
                                        size and orientation); problems of this kind come from
                                        gcr_problem_create_sift_homography */

typedef struct gcr_ctx gcr_ctx;
typedef struct gcr_problem gcr_problem;

/* Mirrors utils::Settings (settings.h:42-74) for the fields the Python entry
 * points set (gcransac_python.cpp:79-85, 191-197, 314-321), plus extensions. */
typedef struct gcr_params {
    double scale_residual_thresh;        /* settings.threshold(0)                         */
    double orientation_residual_thresh;  /* settings.threshold(1) (SIFT only)             */
    double spatial_coherence_weight;     /* lambda; binding default 0.0                   */
    uint64_t min_iteration_number;       /* binding default 10000                         */
    uint64_t max_iteration_number;       /* binding default 10000                         */
    uint64_t max_local_optimization_number; /* binding default 50                        */
    double confidence;                   /* settings.h:60 default 0.95 (not set by Python) */
    uint64_t seed;                       /* extension: Philox key (reference is unseeded) */
    uint32_t batch_slots;                /* extension: outer-iteration slots per launch, 0 = auto */
    uint32_t flags;                      /* GCR_FLAG_*: bit 0 disables local optimisation (bench only), bit 1 the guided stop, bit 2 the PROSAC stop */
    /* extension (homography / fundamental matrix only): the neighbourhood grid
     * over (x1, y1, x2, y2) whose cells give labeling()'s pairwise terms
     * (GridNeighborhoodGraph<4>, grid_neighborhood_graph.h:229-301); cell
     * sizes in pixels, cell_number cells along every axis; 0 = the empty grid
     * of the reference's entry points (no pairwise terms).  A cell size of
     * exactly 0 (ABI 5) is taken from the data: the column's largest finite
     * coordinate + 1 (at least 1) over cell_number, as
     * pygcransac.grid_cell_sizes computes it for an unknown image size */
    double cell_size[4];
    uint32_t cell_number;
    uint32_t reserved;
} gcr_params;

#define GCR_FLAG_NO_LO 1u
/* Guided sampling only (a homography / fundamental-matrix problem with
 * probabilities set; anything else, gcr_solve_batch's items included, is
 * GCR_EINVAL): the adaptive stop uses the best model's inlier MASS, the
 * inliers' share of the sampling weight, in place of its inlier share I / N
 * (csrc/guided_stop.h is the definition).  With all-equal weights the two are
 * the same bits.  Clear (the default): the reference's uniform bound. */
#define GCR_FLAG_GUIDED_STOP 2u
/* PROSAC sampling only (a problem after gcr_problem_set_prosac; anything
 * else -- a uniform or guided problem, the one-shot entries, gcr_solve_batch's
 * items -- and both stop flags together are GCR_EINVAL): the adaptive stop
 * uses the best model's inlier share I_n / n over the best-ranked prefix n*
 * that is non-random and covered by the samples drawn so far, in place of
 * I / N (csrc/prosac_stop.h is the definition).  n* = N is always allowed, so
 * the flag can only lower max_iteration.  Clear (the default): the reference's
 * uniform bound. */
#define GCR_FLAG_PROSAC_STOP 4u

/* model.h: NormalizingTransform{x0,y0,s}, RectifyingHomography{h7,h8},
 * ScaleBased{alpha}, OrientationBased{phi}. */
typedef struct gcr_rect_model {
    double x0, y0, s, h7, h8, alpha, phi;
} gcr_rect_model;

/* utils::RANSACStatistics (statistics.h:43-64) plus per-phase timings. */
typedef struct gcr_stats {
    uint64_t iteration_number;
    uint64_t local_optimization_number;
    uint64_t graph_cut_number;
    uint64_t slots;               /* outer-loop bodies executed                     */
    uint64_t hypotheses;          /* models scored in the main loop                 */
    uint64_t hypotheses_computed; /* models scored on the GPU incl. speculative     */
    uint64_t lo_models;           /* models scored inside local optimisation        */
    uint64_t launches;
    double score;                 /* statistics.score                               */
    double ms_setup, ms_generate, ms_score, ms_replay, ms_lo, ms_refit, ms_total;
    double ms_score_kernel;       /* summed HIP-event time of the scoring kernels   */
    double ms_lo_lists;           /* LO: inlier lists (GPU labeling + copy back)    */
    double ms_lo_fit;             /* LO: sample draws + least-squares fits (host)   */
    double ms_lo_score;           /* LO: scoring the trial models (GPU)             */
    double ms_refit_fit;          /* final refit: the non-minimal fit itself (system,
                                     QR, weighted mode); the rest of ms_refit is the
                                     buffer reconciliation, rescoring and lists      */
    uint64_t prefetched_chunks;   /* chunks generated + scored on the side stream
                                     while the host replayed the previous one        */
    /* decisions in the reference's arithmetic (glibc; csrc/exact.h): the kernels
     * flag every decision whose detmath residual lies within the proven
     * twin-glibc bound of its threshold, and the host takes it with glibc */
    uint64_t exact_models;        /* models rescored / relabelled on the host       */
    uint64_t exact_pairs;         /* (feature, model) decisions taken with glibc    */
    uint64_t exact_flips;         /* ... that differ from the detmath decision      */
    double ms_exact;              /* host time of those recounts                    */
    /* score comparisons in glibc (exact.h ScoreBound): two value scores closer
     * than their proven bounds are compared by their glibc scores */
    uint64_t near_ties;           /* comparisons decided in glibc                   */
    uint64_t near_tie_flips;      /* ... whose outcome differs from the values'     */
    /* LO trials are compared on approximate scores within a proven bound of
     * the exact ones; a round the bound leaves open is folded exactly */
    uint64_t lo_refolds;          /* LO rounds folded exactly for a comparison      */
    /* the final refit's inlier lists decoded from the MSAC ballots of the
     * chunk launch that found the best (1) instead of mask launches (0) */
    uint64_t chunk_msac_lists;
} gcr_stats;

/* ---- context ---------------------------------------------------------- */
const char* gcr_last_error(void);
int gcr_abi_version(void);
int gcr_device_count(void);
/* SHA-256 prefix (16 hex) of the sources the GPU code object was built from
 * (kernels.hip + device headers + build flags); profiles are keyed by it */
const char* gcr_kernel_build_id(void);
int gcr_create(int device, gcr_ctx** out);
void gcr_destroy(gcr_ctx* ctx);
/* hipDeviceSynchronize on the context's device */
int gcr_synchronize(gcr_ctx* ctx);
void gcr_default_params(gcr_params* p);

/* ---- drop-in entry points (one call = one reference call) ---------------- */
int gcr_rect_scale_only(gcr_ctx* ctx, const double* features, size_t n, const gcr_params* params, int original,
                        uint8_t* mask_out, double* H_out, gcr_rect_model* model_out, gcr_stats* stats_out);

int gcr_rect_sift(gcr_ctx* ctx, const double* scale_features, size_t n_scale, const double* orientation_features,
                  size_t n_orientation, const gcr_params* params, uint8_t* scale_mask_out,
                  uint8_t* orientation_mask_out, double* H_out, gcr_rect_model* model_out, gcr_stats* stats_out);

/* 4-point homography (an EXTENSION: this fork has no
 * homography estimator, finding 0.1 -- the entry point upstream pygcransac's
 * findHomography would bind).  correspondences: row-major N x 4 float64
 * (x1, y1, x2, y2); threshold = params->scale_residual_thresh (pixels, second
 * image); mask_out: N bytes; H_out: row-major 3x3 with H[2][2] = 1.  Returns
 * the number of inliers (0: no model, H_out untouched) or < 0 on error. */
int gcr_find_homography(gcr_ctx* ctx, const double* correspondences, size_t n, const gcr_params* params,
                        uint8_t* mask_out, double* H_out, gcr_stats* stats_out);

/* 7-point fundamental matrix (an EXTENSION like
 * gcr_find_homography -- what upstream pygcransac's findFundamentalMatrix
 * would bind).  Same buffers as gcr_find_homography; the residual is the
 * squared Sampson distance, F_out is row-major 3x3 with unit Frobenius norm
 * (x2^T F x1 = 0). */
int gcr_find_fundamental_matrix(gcr_ctx* ctx, const double* correspondences, size_t n, const gcr_params* params,
                                uint8_t* mask_out, double* F_out, gcr_stats* stats_out);

/* Guided (importance) sampling, upstream GC-RANSAC's sampler 3: the one-shot
 * entries above with per-correspondence sampling weights, `probabilities`
 * (n float64, each finite and >= 0, at least 4 / 7 of them > 0, a finite sum;
 * anything else is GCR_EINVAL).  Every minimal sample of the main loop draws
 * correspondence i with probability w[i] / sum(w) (csrc/guided.h is the
 * definition); a zero weight is never drawn.  Validity checks, solvers,
 * scoring and local optimisation (whose inner sampler stays uniform) are
 * unchanged.  The adaptive stop is the reference's uniform bound on I / N
 * unless params->flags has GCR_FLAG_GUIDED_STOP: then it is the same formula
 * on the best model's inlier mass W_I / W (csrc/guided_stop.h), which ends a
 * run with informative weights as soon as its own sampler justifies it.
 * probabilities == NULL: exactly the plain entry (the flag is then GCR_EINVAL). */
int gcr_find_homography_guided(gcr_ctx* ctx, const double* correspondences, size_t n, const double* probabilities,
                               const gcr_params* params, uint8_t* mask_out, double* H_out, gcr_stats* stats_out);
int gcr_find_fundamental_matrix_guided(gcr_ctx* ctx, const double* correspondences, size_t n,
                                       const double* probabilities, const gcr_params* params, uint8_t* mask_out,
                                       double* F_out, gcr_stats* stats_out);

/* 5-point essential matrix for calibrated cameras (an EXTENSION like the two
 * above -- what upstream pygcransac's findEssentialMatrix would bind;
 * csrc/ess.h is the definition).  correspondences: N x 4 PIXEL rows; K1, K2:
 * row-major 3 x 3 calibration matrices, every entry finite, third row exactly
 * (0, 0, 1), K[1][0] == 0, K[0][0] and K[1][1] > 0 (skew allowed); anything
 * else, and n < 5, is GCR_EINVAL.  The estimator runs on x^ = K^-1 x (closed
 * form, fp64) with the squared Sampson distance;
 * params->scale_residual_thresh is in pixels and is divided by
 * (K1[0][0] + K1[1][1] + K2[0][0] + K2[1][1]) / 4 (upstream's rule).  The
 * neighbourhood grid of params (cell sizes in pixels) lies over the pixel
 * rows.  probabilities: NULL = uniform sampling, else guided as in
 * gcr_find_fundamental_matrix_guided (at least 5 weights > 0).  E_out:
 * row-major 3 x 3, unit Frobenius norm, x^2^T E x^1 = 0. */
int gcr_find_essential_matrix(gcr_ctx* ctx, const double* correspondences, size_t n, const double* K1,
                              const double* K2, const double* probabilities, const gcr_params* params,
                              uint8_t* mask_out, double* E_out, gcr_stats* stats_out);

/* 3-point essential matrix for calibrated cameras whose gravity direction is
 * known (an EXTENSION -- what upstream pygcransac's findGravityEssentialMatrix
 * would bind; parity with upstream is unpinned, csrc/grav.h is the
 * definition).  Everything as gcr_find_essential_matrix, plus G1
 * (gravity_source) and G2 (gravity_destination): row-major 3 x 3 rotations,
 * Gi taking a direction in camera i to a frame whose y axis is the gravity
 * direction.  They must be finite with |G G^T - I|_max <= 1e-9 and det > 0;
 * anything else is GCR_EINVAL with a message naming gravity_source or
 * gravity_destination, before any GPU work.  n < 3 is GCR_EINVAL.  A sample
 * is three correspondences and yields up to four models; probabilities need
 * at least 3 weights > 0.  The relative rotation must not be a half turn about
 * the vertical in the aligned frames (outside the solver's parametrisation).
 * E_out: as gcr_find_essential_matrix's, in the ordinary normalised frames
 * (x^2^T E x^1 = 0), of the form G2^T [t]x R_y G1. */
int gcr_find_gravity_essential_matrix(gcr_ctx* ctx, const double* correspondences, size_t n, const double* K1,
                                      const double* K2, const double* G1, const double* G2,
                                      const double* probabilities, const gcr_params* params, uint8_t* mask_out,
                                      double* E_out, gcr_stats* stats_out);

/* Homography from two SIFT correspondences (an EXTENSION -- what upstream
 * pygcransac's findHomography binds as its SIFT-based solver; parity with
 * upstream is unpinned, csrc/sifth.h is the definition).  correspondences:
 * N x 4 rows x1, y1, x2, y2 in pixels; sift: N x 4 rows q1, q2, alpha1,
 * alpha2 -- the feature sizes as lengths (any fixed multiple of them on both
 * sides) and the orientations in radians.  A q that is not finite and > 0 or
 * an alpha that is not finite is GCR_EINVAL with a message naming the column
 * (q1, q2, alpha1, alpha2), before any GPU work; n < 4 is GCR_EINVAL.  A
 * sample is two correspondences and yields up to three models; scoring, the
 * inlier threshold, local optimisation (its fits are the 4-point estimator's
 * non-minimal fit, on samples of up to 14), the neighbourhood grid and H_out
 * (H[8] = 1) are gcr_find_homography's.  probabilities: NULL (uniform) or n
 * weights with at least 2 of them > 0 (guided, as
 * gcr_find_homography_guided).  A minimal model covers few inliers (an
 * orientation error is multiplied by the distance from the sample), so the
 * estimator rests on local optimisation: GCR_FLAG_NO_LO makes little sense
 * here. */
int gcr_find_homography_sift(gcr_ctx* ctx, const double* correspondences, const double* sift, size_t n,
                             const double* probabilities, const gcr_params* params, uint8_t* mask_out, double* H_out,
                             gcr_stats* stats_out);

/* ---- batches of independent problems (SURVEY.md §8(b) gcr_rect_batch,
 * BASELINE configs[4]) ----------------------------------------------------- */
typedef struct gcr_batch_item {
    int solver;                  /* GCR_SOLVER_*                                   */
    const double* f0;            /* N0 x 3 features, or N0 x 4 correspondences     */
    size_t n0;
    const double* f1;            /* orientation features (SIFT22), else NULL       */
    size_t n1;
    gcr_params params;
    uint8_t* mask0_out;          /* caller-owned, n0 bytes                          */
    uint8_t* mask1_out;          /* caller-owned, n1 bytes (SIFT22), else NULL      */
    double H_out[9];
    gcr_rect_model model_out;
    gcr_stats stats_out;
    int result;                  /* inlier count (0: no model) or error code        */
} gcr_batch_item;
/* Solve n independent problems on one device.  `concurrency` host threads,
 * each with its own context (HIP stream + workspace), take problems from a
 * shared counter, longest first (estimated from the solver and the feature
 * count), so one problem's host phases (replay, LO fits, refit control)
 * overlap another's kernels and the batch does not end on a long problem
 * started last.  Results are per item; returns
 * GCR_OK, or the first error code (message in gcr_last_error()). */
int gcr_solve_batch(int device, gcr_batch_item* items, size_t n, int concurrency);

/* ---- device-resident problems (benchmarks, problem batches) -------------- */
/* Uploads the features once; runs reuse the HBM-resident copy.  f1 is the
 * orientation set for GCR_SOLVER_SIFT22 and NULL otherwise. */
int gcr_problem_create(gcr_ctx* ctx, int solver, const double* f0, size_t n0, const double* f1, size_t n1,
                       gcr_problem** out);
/* A resident essential-matrix problem (GCR_SOLVER_ESSENTIAL5) from pixel
 * rows and calibration matrices, checked as gcr_find_essential_matrix checks
 * them.  gcr_problem_create(5, ...) carries no calibration and is GCR_EINVAL,
 * as are essential items of gcr_solve_batch.  gcr_problem_run, _run_sharded,
 * _run_comm, _verify_batch(es), _set_probabilities and the *_h debug hooks
 * accept the problem; thresholds in their params are in pixels, models passed
 * to or from the debug hooks are in normalised coordinates. */
int gcr_problem_create_essential(gcr_ctx* ctx, const double* correspondences, size_t n, const double* K1,
                                 const double* K2, gcr_problem** out);
/* The same for the essential matrix with known gravity
 * (GCR_SOLVER_ESSENTIAL3_GRAVITY): an essential problem plus the two rotations,
 * checked as gcr_find_gravity_essential_matrix checks them.
 * gcr_problem_create(6, ...) and items of gcr_solve_batch of kind 6 are
 * GCR_EINVAL; everything the essential problem is accepted by accepts this one. */
int gcr_problem_create_gravity_essential(gcr_ctx* ctx, const double* correspondences, size_t n, const double* K1,
                                         const double* K2, const double* G1, const double* G2, gcr_problem** out);
/* A homography problem plus the SIFT columns (GCR_SOLVER_HOMOGRAPHY2_SIFT),
 * checked as gcr_find_homography_sift checks them.  n >= 2 is accepted (the
 * generator and sampler hooks work on it); the run entries -- gcr_problem_run,
 * _run_sharded, _run_comm, _verify_batch(es) -- need n >= 4 and are GCR_EINVAL
 * below that.  gcr_problem_create(7, ...) and items of gcr_solve_batch of kind
 * 7 are GCR_EINVAL; everything the homography problem is accepted by accepts
 * this one (gcr_problem_set_probabilities: at least 2 weights > 0). */
int gcr_problem_create_sift_homography(gcr_ctx* ctx, const double* correspondences, const double* sift, size_t n,
                                       gcr_problem** out);
void gcr_problem_destroy(gcr_problem* prob);
/* Guided sampling for a resident homography / fundamental-matrix problem (see
 * gcr_find_homography_guided): n must be the problem's N.  Everything that
 * generates from the problem afterwards -- gcr_problem_run, _run_sharded,
 * _run_comm, _verify_batch(es), gcr_debug_generate_h -- draws its samples
 * with these weights.  probabilities == NULL (n ignored) returns the problem
 * to uniform sampling.  Either call first waits for a speculative chunk a
 * previous run left in flight.  Rectification problems: GCR_EINVAL.
 * gcr_solve_batch's items carry no probabilities and stay uniform. */
int gcr_problem_set_probabilities(gcr_problem* prob, const double* probabilities, size_t n);
/* PROSAC sampling (upstream's sampler 1; csrc/prosac.h is the definition)
 * for a resident correspondence problem -- every solver the guided sampler is
 * valid for.  The problem's rows must be in quality order, best first.  Early
 * slots draw from the best-ranked rows, the pool grows on a fixed schedule of
 * `convergence_iterations` (T_N; 1 .. 2^40, upstream's default is 100000) and
 * past it every slot draws the uniform sampler's own sample.  The pool is a
 * function of the slot index alone, so runs stay bit-identical across
 * batch_slots, shards and ranks.  Everything that generates from the problem
 * afterwards -- gcr_problem_run, _run_sharded, _run_comm, _verify_batch(es),
 * gcr_debug_generate_h, gcr_debug_sample_h, gcr_measure_generate_h -- uses
 * it; local optimisation's inner sampler stays uniform and the stop is the
 * uniform bound unless params->flags has GCR_FLAG_PROSAC_STOP: then it is
 * PROSAC's own non-randomness / maximality stop (csrc/prosac_stop.h), whose
 * Imin table is built here.  convergence_iterations == 0 returns the problem to uniform
 * sampling.  Either call first waits for a speculative chunk a previous run
 * left in flight.  GCR_EINVAL, the problem left as it was: rectification
 * problems, convergence_iterations > 2^40, a problem with probabilities set
 * (guided and PROSAC sampling are exclusive: clear one first; likewise
 * gcr_problem_set_probabilities on a PROSAC problem).  GCR_FLAG_GUIDED_STOP on
 * a PROSAC problem is GCR_EINVAL, as is GCR_FLAG_PROSAC_STOP on any other.
 * gcr_solve_batch's items stay uniform. */
int gcr_problem_set_prosac(gcr_problem* prob, uint64_t convergence_iterations);
/* NAPSAC sampling (upstream's sampler 2, progressive NAPSAC; csrc/napsac.h is
 * the definition) for a resident correspondence problem of any of the five
 * solvers.  It needs no scores, only the positions: a slot below
 * `local_iterations` (T; 1 .. 2^40) draws its first row uniformly and the
 * others from that row's cell of a grid over (x1, y1, x2, y2) -- 16, 8, 4,
 * then 2 cells per axis in the four quarters of T, the next coarser layer
 * where the cell holds fewer rows than a minimal sample -- and every slot
 * from T on draws the uniform sampler's own sample.  `extent` = {w1, h1, w2,
 * h2}, positive and finite: the image sizes the grids divide (an unknown size:
 * the data's extent, as pygcransac.grid_cell_sizes computes it).  The layers
 * are built on the host from the problem's pixel columns and uploaded; a
 * slot's sample is a function of (seed, slot, attempt) alone, so runs stay
 * bit-identical across batch_slots, shards and ranks.  Everything that
 * generates from the problem afterwards -- gcr_problem_run, _run_sharded,
 * _run_comm, _verify_batch(es), gcr_debug_generate_h, gcr_debug_sample_h,
 * gcr_measure_generate_h -- uses it; local optimisation's inner sampler stays
 * uniform and the stop is the uniform bound: what it describes from slot T on,
 * and applied before T too, where it is a heuristic (a run whose bound falls
 * below T ends inside the local phase).  local_iterations == 0 returns
 * the problem to uniform sampling (extent is then not read).  Either call
 * first waits for a speculative chunk a previous run left in flight.
 * GCR_EINVAL, the problem left as it was: rectification problems, bad extents,
 * local_iterations > 2^40, a problem with probabilities or PROSAC set (the
 * three samplers are exclusive: clear one first; likewise
 * gcr_problem_set_probabilities and gcr_problem_set_prosac on a NAPSAC
 * problem).  GCR_FLAG_GUIDED_STOP or GCR_FLAG_PROSAC_STOP on a NAPSAC problem
 * is GCR_EINVAL.  gcr_solve_batch's items stay uniform. */
int gcr_problem_set_napsac(gcr_problem* prob, const double extent[4], uint64_t local_iterations);
/* full estimator call on the resident problem (same semantics as gcr_rect_*) */
int gcr_problem_run(gcr_problem* prob, const gcr_params* params, uint8_t* mask0_out, uint8_t* mask1_out,
                    double* H_out, gcr_rect_model* model_out, gcr_stats* stats_out);

/* One problem over `world` processes: every rank
 * calls this with the same problem and params.  Each fetched chunk of slots is
 * split into `world` contiguous blocks; rank r generates and scores block r
 * on its own device, and `allgather` (host memory: `bytes` from every rank
 * into recv, rank-major -- e.g. RCCL all_gather over xGMI, or gloo) hands
 * every rank the whole chunk.  The replay, LO and the final refit then run
 * identically on every rank, so all ranks return the single-rank result bit
 * for bit.  The callback returns 0 on success. */
typedef int (*gcr_allgather_fn)(void* user, const void* send, void* recv, size_t bytes);
int gcr_problem_run_sharded(gcr_problem* prob, const gcr_params* params, int rank, int world,
                            gcr_allgather_fn allgather, void* user, uint8_t* mask0_out, uint8_t* mask1_out,
                            double* H_out, gcr_rect_model* model_out, gcr_stats* stats_out);

/* The same run with the exchange inside the engine: a communicator rank
 * (RCCL over xGMI, one process per GPU) all-gathers the device-resident block
 * summaries with ncclAllGather on the context's side stream, behind the
 * summary kernel -- no host callback, no host staging of the send side, one
 * copy of the gathered records into pinned memory.  gcr_comm_unique_id on one
 * rank, the id handed to every rank (e.g. a torch.distributed broadcast),
 * then gcr_comm_create on every rank (collective). */
#define GCR_COMM_ID_BYTES 128
typedef struct gcr_comm gcr_comm;
int gcr_comm_unique_id(uint8_t id_out[GCR_COMM_ID_BYTES]);
int gcr_comm_create(gcr_ctx* ctx, int rank, int world, const uint8_t id[GCR_COMM_ID_BYTES], gcr_comm** out);
void gcr_comm_destroy(gcr_comm* comm);
int gcr_problem_run_comm(gcr_problem* prob, const gcr_params* params, gcr_comm* comm, uint8_t* mask0_out,
                         uint8_t* mask1_out, double* H_out, gcr_rect_model* model_out, gcr_stats* stats_out);

/* One pass of the hot path over one batch: draw and solve `nslots`
 * outer-iteration slots starting at `slot0`, MSAC-score every resulting model
 * against all features on the GPU, and return the best-scoring slot (first
 * strict maximum of the reference's update rule, `best < score &&
 * isValidModel`, GCRANSAC.h:440-446).  This is the throughput API of the hot
 * path: the rectification solvers' scores, inlier decisions and the 2-SIFT
 * best_model's phi are the kernels' own (the detmath twins, csrc/exact.h),
 * with no host recheck of flagged decisions or near-tie comparisons, so a
 * batch whose best is decided within the twin-glibc bounds can differ from
 * the reference's choice.  gcr_problem_run (and the pygcransac entry points)
 * take every decision, comparison and model in the reference's arithmetic.
 * Timings go to stats_out. */
typedef struct gcr_batch_result {
    uint64_t models;        /* hypotheses scored                        */
    uint64_t iterations;    /* sum of iteration increments of the batch */
    int64_t best_slot;      /* -1 if no model scored > 0                */
    double best_score;
    uint64_t best_inliers[2];
    gcr_rect_model best_model;
} gcr_batch_result;
int gcr_problem_verify_batch(gcr_problem* prob, const gcr_params* params, uint64_t slot0, uint32_t nslots,
                             gcr_batch_result* out, gcr_stats* stats_out);
/* `nbatches` consecutive batches of `nslots` slots (batch b covers slots
 * slot0 + b*nslots ...), queued back to back on the device with the per-batch
 * selection done on the GPU; out[] holds one result per batch.  One host
 * synchronisation per call.  Returns GCR_OK or an error code. */
int gcr_problem_verify_batches(gcr_problem* prob, const gcr_params* params, uint64_t slot0, uint32_t nslots,
                               uint32_t nbatches, gcr_batch_result* out, gcr_stats* stats_out);

/* ---- many small problems per call (csrc/verify_many.h is the definition) -- */
/* The best hypothesis of `nproblems` independent small correspondence problems
 * in one call: a fixed number of launches for all of them, one upload, one
 * synchronisation, one download.  solver is GCR_SOLVER_HOMOGRAPHY4 or
 * GCR_SOLVER_FUNDAMENTAL7, for the whole call.  rows holds every problem's
 * N x 4 rows (x1, y1, x2, y2) back to back; problem p owns rows
 * row_offset[p] .. row_offset[p + 1] - 1 (row_offset: nproblems + 1 ascending
 * values, at least 4 / 7 rows per problem, fewer than 2^32 rows in all),
 * thresholds[p] is its inlier threshold in pixels and seeds[p] its sampler
 * seed.  out[p] is what gcr_problem_verify_batch(prob, params, 0, nslots)
 * returns for a resident problem of those rows alone with uniform sampling,
 * params.seed = seeds[p] and params.scale_residual_thresh = thresholds[p]:
 * models, iterations, the best slot (-1: no hypothesis scored above 0) and its
 * score and inlier count, plus the hypothesis inside the slot (0 for the
 * homography, 0 .. 2 for the fundamental matrix) and its own nine doubles
 * (gcr_debug_generate_h's, row-major; the default model 1 0 0 0 1 0 0 0 1
 * without a best).  masks_out (may be NULL): row_offset[nproblems] bytes, row
 * i's inlier decision under best_model by gcr_debug_mask_h's rule 0, all zero
 * for a problem without a best; a problem's bytes sum to best_inliers.  The
 * device result equals gcr_host_verify_many's byte for byte, for every
 * GCR_MANY_BLOCK (64, 128 or 256 slots per workgroup; read per call, tests).
 * GCR_EINVAL with a message naming the argument, before any GPU work (so also
 * with a NULL context): a NULL array, another solver, nproblems == 0, offsets
 * that do not start at 0 or descend, a problem with too few rows, 2^32 rows or
 * more, a non-finite row, a threshold that is not finite and > 0, nslots
 * outside 1 .. 65536.  ms_kernel_out may be NULL: HIP-event time of the
 * kernels. */
typedef struct gcr_many_result {
    uint64_t models, iterations;
    int64_t  best_slot;
    uint32_t best_hypothesis, best_inliers;
    double   best_score;
    double   best_model[9];
} gcr_many_result;
int gcr_verify_many(gcr_ctx* ctx, int solver, const double* rows, const uint64_t* row_offset, size_t nproblems,
                    const double* thresholds, const uint64_t* seeds, uint32_t nslots, gcr_many_result* out,
                    uint8_t* masks_out, double* ms_kernel_out);
/* host-only: the same by plain loops (no GPU); `threads` (clamped to 1..16)
 * splits the problems only and does not change the result */
int gcr_host_verify_many(int solver, const double* rows, const uint64_t* row_offset, size_t nproblems,
                         const double* thresholds, const uint64_t* seeds, uint32_t nslots, int threads,
                         gcr_many_result* out, uint8_t* masks_out);

/* ---- parity / debug hooks (used by tests; GPU required unless noted) ---- */
/* inc[i] in 1..101 (attempt of success) or 102 (no model), models[i] */
int gcr_debug_generate(gcr_problem* prob, uint64_t seed, uint64_t slot0, uint32_t nslots, uint8_t* inc_out,
                       gcr_rect_model* models_out);
/* raw MSAC accumulators for explicit models: counts, per-class sums, total */
int gcr_debug_score(gcr_problem* prob, const gcr_params* params, const gcr_rect_model* models, uint32_t nmodels,
                    uint32_t* n0, uint32_t* n1, double* v0, double* v1, double* tot);
/* every slot of one fused generate + score launch (rectification solvers): what
 * a one-batch gcr_problem_verify_batches call launches (unchained, one group),
 * without its selection.  inc_out[i] as gcr_debug_generate's, the raw MSAC
 * accumulators as gcr_debug_score's (zeros for a slot without a model); the
 * sampler seed is params->seed */
int gcr_debug_verify_slots(gcr_problem* prob, const gcr_params* params, uint64_t slot0, uint32_t nslots,
                           uint8_t* inc_out, uint32_t* n0, uint32_t* n1, double* v0, double* v1, double* tot);
/* The bound path of gcr_problem_verify_batches (rectification solvers, calls
 * of at least 4 batches; GCR_VERIFY_BOUND=0 or a set A/B switch of the fused
 * path disables it): the same launches as that call's, returning per slot the
 * features that pass the conservative pre-band -- ub0_out / ub1_out,
 * nbatches * nslots entries each, upper bounds of the slot's inlier counts, 0
 * for a slot without a model -- and per batch in scored_out[nbatches] how many
 * slots were scored exactly.  The hook bounds every slot with a model, as
 * GCR_VERIFY_BOUND_LIVE=0 does; the records and scored_out do not depend on
 * that.  GCR_EINVAL when the call would not take the bound path. */
int gcr_debug_verify_bound(gcr_problem* prob, const gcr_params* params, uint64_t slot0, uint32_t nslots,
                           uint32_t nbatches, uint32_t* ub0_out, uint32_t* ub1_out, uint32_t* scored_out);
/* The same call in the default mode, whatever GCR_VERIFY_BOUND_LIVE says:
 * walked_out[nbatches], per batch the slots on the live list, i.e. those whose
 * bounds k_bound counted -- the slots with a model and, for the 2-SIFT solver,
 * a valid one.  GCR_EINVAL as above. */
int gcr_debug_verify_bound_live(gcr_problem* prob, const gcr_params* params, uint64_t slot0, uint32_t nslots,
                                uint32_t nbatches, uint32_t* walked_out);
/* The run loop's score comparison `score(a) < score(b)` (GCRANSAC.h:440) as
 * gcr_problem_run takes it: both models scored by the GPU small scorer (value
 * scores), compared directly when they are further apart than their proven
 * value-glibc bounds (csrc/exact.h ScoreBound), else by their glibc scores
 * recounted on the host.  Returns bit 0 the decision, bit 1 a near tie, bit 2
 * the value scores' own order; < 0 an error. */
int gcr_debug_score_less(gcr_problem* prob, const gcr_params* params, const gcr_rect_model* a,
                         const gcr_rect_model* b);
/* With GCR_EXCHANGE_LOG=1, the summary replay of the last run on the calling
 * thread logs every event that is a collective under gcr_comm (chunk issue,
 * re-summary) and every chunk it collected: 4 words per event (engine.cpp
 * t_xlog).  Copies min(count, cap) words to out (may be null); returns the
 * count.  No GPU needed. */
size_t gcr_debug_exchange_log(uint64_t* out, size_t cap);
/* inlier mask of one model: rule 0 = MSAC (2.25 thr^2), 1 = LO threshold
 * ((1.5 thr)^2), 2 = 1-class graph-cut labeling */
int gcr_debug_mask(gcr_problem* prob, const gcr_params* params, const gcr_rect_model* model, int cls, int rule,
                   uint8_t* mask_out);
/* the LO / final-refit fit of the given index lists on the problem's features;
 * use_gpu = 1 solves the hybrid least-squares system with the GPU refit path
 * (k_sift_rows + device QR), 0 on the host; both are bit-identical.  Returns 1
 * and the model, 0 if the fit is rejected, < 0 on error */
int gcr_debug_fit_nonminimal(gcr_problem* prob, const uint32_t* idx0, size_t k0, const uint32_t* idx1, size_t k1,
                             int use_gpu, gcr_rect_model* model_out);
/* host-only (no GPU): the LO / final-refit least-squares fit of the given index
 * lists (RectifyingHomographyEstimator::estimateModelNonminimal,
 * rectifying_homography_estimator.h:164-227); returns 1 and the model, 0 if the
 * fit is rejected, < 0 on error */
int gcr_host_fit_nonminimal(int solver, const double* f0, size_t n0, const double* f1, size_t n1, const uint32_t* idx0,
                            size_t k0, const uint32_t* idx1, size_t k1, gcr_rect_model* model_out);
/* correspondence problems (GCR_SOLVER_HOMOGRAPHY4 / _FUNDAMENTAL7): models
 * are 9 row-major doubles.  generate: homography -- inc[i] as above, H_out 9
 * per slot; fundamental -- 3 hypotheses per slot (inc_out 3 bytes, H_out 27
 * doubles per slot): inc[3s] as above, inc[3s+k] = 0 if the sample's k-th
 * model exists, 255 if not; essential -- the same with 10 hypotheses per slot
 * (inc_out 10 bytes, H_out 90 doubles per slot), gravity essential with 4
 * (4 bytes, 36 doubles), SIFT homography with 3 (3 bytes, 27 doubles).  score: n0 / v0 / tot per model (MSAC threshold
 * 2.25 thr); mask: rules as gcr_debug_mask */
int gcr_debug_generate_h(gcr_problem* prob, uint64_t seed, uint64_t slot0, uint32_t nslots, uint8_t* inc_out,
                         double* H_out);
/* the generators' sampling function alone: the 4 / 7 / 5 / 3 / 2 (solvers 3 .. 7)
 * indices of attempt `attempt` of slots slot0 .. slot0 + nslots - 1 (idx_out:
 * as many per slot,
 * all-ones where the draw budget ran out), with the problem's sampler --
 * guided after gcr_problem_set_probabilities, PROSAC after
 * gcr_problem_set_prosac, NAPSAC after gcr_problem_set_napsac, else uniform */
int gcr_debug_sample_h(gcr_problem* prob, uint64_t seed, uint64_t slot0, uint32_t nslots, uint32_t attempt,
                       uint32_t* idx_out);
/* measurement (tools/guided_bench.py): HIP-event time per launch, in ms, of
 * `reps` back-to-back generator launches of nslots slots each (consecutive
 * slot ranges from slot0) with the problem's sampler, after one untimed launch */
int gcr_measure_generate_h(gcr_problem* prob, uint64_t seed, uint64_t slot0, uint32_t nslots, int reps,
                           double* ms_out);
/* host-only: the generators' validity check + minimal solver on the listed
 * rows (4: valid_sample_h4 + solve_h4; 7: solve_f7_basis + f7_model), in list
 * order, the functions the kernels call.  *count_out = 0 .. 3 models, 9
 * doubles each in models_out (room for 27).  Solver 5: solve_e5 on NORMALISED
 * rows, *count_out = 0 .. 10 models: models_out needs room for 90 doubles. */
int gcr_host_solve_minimal(int solver, const double* correspondences, size_t n, const uint32_t* idx,
                           double* models_out, uint32_t* count_out);
int gcr_debug_score_h(gcr_problem* prob, const gcr_params* params, const double* H, uint32_t nmodels, uint32_t* n0,
                      double* v0, double* tot);
int gcr_debug_mask_h(gcr_problem* prob, const gcr_params* params, const double* H, int rule, uint8_t* mask_out);
/* the guided stop's kernel alone (csrc/guided_stop.h) on a problem with
 * probabilities set: per model of H (9 doubles each) the number of
 * correspondences within the MSAC threshold 2.25 thr^2 (equal to
 * gcr_debug_score_h's n0) and the sum of their quanta */
int gcr_debug_inlier_mass_h(gcr_problem* prob, const gcr_params* params, const double* H, uint32_t nmodels,
                            uint32_t* count_out, uint64_t* mass_out);
/* the PROSAC stop's kernel alone (csrc/prosac_stop.h) on a problem that
 * samples with PROSAC, at params' threshold and confidence: per model of H (9
 * doubles each) the number of correspondences within the MSAC threshold
 * 2.25 thr^2 (equal to gcr_debug_score_h's n0) and the chosen prefix
 * (I*, n*) */
int gcr_debug_prosac_stop_h(gcr_problem* prob, const gcr_params* params, const double* H, uint32_t nmodels,
                            uint32_t* count_out, uint32_t* best_i_out, uint32_t* best_n_out);
/* host-only: normalised least-squares homography of the listed
 * correspondences (the LO / final-refit fit); 1 = fitted, 0 = rejected */
int gcr_host_fit_h(const double* correspondences, size_t n, const uint32_t* idx, size_t k, double* H_out);
/* host-only: the fundamental-matrix LO / refit fit (7 points: 7-point solver's
 * first model; more: normalised 8-point with rank-2 projection) */
int gcr_host_fit_f(const double* correspondences, size_t n, const uint32_t* idx, size_t k, double* F_out);
/* host-only: the essential-matrix LO / refit fit on NORMALISED rows (5 points:
 * the 5-point solver's first model; more: the four smallest eigenvectors of
 * A^T A through ess.h's steps 3-7, the candidate with the smallest Sampson
 * sum) */
int gcr_host_fit_e(const double* correspondences_normalised, size_t n, const uint32_t* idx, size_t k, double* E_out);
/* host-only: the host twin of the essential-matrix generator with uniform
 * draws, over `threads` host threads: gcr_debug_generate_h's inc_out (10 bytes
 * per slot) and models (90 doubles per slot) of NORMALISED rows, bit for bit
 * (measurements' CPU baseline; tests) */
int gcr_host_generate_e(const double* correspondences_normalised, size_t n, uint64_t seed, uint64_t slot0,
                        uint32_t nslots, int threads, uint8_t* inc_out, double* models_out);
/* host-only: what an essential-matrix problem holds: normalised_out (N x 4) =
 * the rows K-normalised, *threshold_out (may be NULL) = the pixel threshold
 * in normalised units; K1 / K2 checked as gcr_find_essential_matrix does */
int gcr_host_essential_normalise(const double* correspondences, size_t n, const double* K1, const double* K2,
                                 double threshold, double* normalised_out, double* threshold_out);
/* host-only, essential matrix with known gravity (csrc/grav.h).  The rotations
 * are checked as gcr_find_gravity_essential_matrix checks them.
 * check_gravity: that check alone.
 * solve_g3: the 3-point solver on the three listed NORMALISED rows
 * (gcr_host_solve_minimal(6, ...) cannot carry the rotations and is
 * GCR_EINVAL): *count_out = 0 .. 4 models in ascending root order, 9 doubles
 * each, models_out needs room for 36.
 * fit_g: the LO / refit fit (3 or 4 rows: the solver's first model; more: the
 * constrained null vector, csrc/host_fit.h); returns 1 with E_out, 0 without a
 * model.
 * generate_g: the host twin of the generator, over `threads` host threads:
 * gcr_debug_generate_h's inc_out (4 bytes per slot) and models (36 doubles per
 * slot) bit for bit; probabilities NULL = uniform draws, else guided (n
 * weights). */
int gcr_host_check_gravity(const double* G1, const double* G2);
int gcr_host_solve_g3(const double* correspondences_normalised, size_t n, const uint32_t* idx, const double* G1,
                      const double* G2, double* models_out, uint32_t* count_out);
int gcr_host_fit_g(const double* correspondences_normalised, size_t n, const uint32_t* idx, size_t k,
                   const double* G1, const double* G2, double* E_out);
int gcr_host_generate_g(const double* correspondences_normalised, size_t n, const double* G1, const double* G2,
                        const double* probabilities, uint64_t seed, uint64_t slot0, uint32_t nslots, int threads,
                        uint8_t* inc_out, double* models_out);
/* host-only, homography from two SIFT correspondences (csrc/sifth.h).
 * correspondences: N x 4 pixel rows; sift: N x 4 rows q1, q2, alpha1, alpha2.
 * check_sift: gcr_find_homography_sift's check of the columns alone.
 * solve_s2: the 2-point solver on the two listed rows (their SIFT entries are
 * checked; gcr_host_solve_minimal(7, ...) cannot carry the columns and is
 * GCR_EINVAL): *count_out = 0 .. 3 models in ascending root order, 9 doubles
 * each, models_out needs room for 27.
 * generate_s: the host twin of the generator, over `threads` host threads:
 * gcr_debug_generate_h's inc_out (3 bytes per slot) and models (27 doubles per
 * slot) bit for bit; probabilities NULL = uniform draws, else guided (n
 * weights). */
int gcr_host_check_sift(const double* sift, size_t n);
int gcr_host_solve_s2(const double* correspondences, const double* sift, size_t n, const uint32_t* idx,
                      double* models_out, uint32_t* count_out);
int gcr_host_generate_s(const double* correspondences, const double* sift, size_t n, const double* probabilities,
                        uint64_t seed, uint64_t slot0, uint32_t nslots, int threads, uint8_t* inc_out,
                        double* models_out);
/* host-only: RectifyingHomography::getHomography (model.h:211-226), row-major */
void gcr_host_homography(const gcr_rect_model* model, double* H_out);
/* host-only: squared residuals of one rectification model over n features of
 * class `cls` (0 scale, 1 orientation; solver 0-2), rows as the entry points
 * take them (x, y, scale | angle).  arith 0: the product's values (rect.h
 * scale_sq_value / orient_sq_value, what the kernels evaluate and fold);
 * 1: the reference's formulas in glibc (the decisions, exact.h). */
int gcr_host_residuals(int solver, int cls, const double* features, size_t n, const gcr_rect_model* model, int arith,
                       double* r2_out);
/* host-only (no GPU): the graph-cut labeling's pieces (graphcut.h).
 * grid_edges: the neighbourhood grid's edges over n points of `dims` (<= 4)
 * row-major coordinates in labeling()'s order (GCRANSAC.h:821-857,
 * grid_neighborhood_graph.h:229-301); writes min(m, cap) pairs, *m_out = m.
 * bk_energy: BK st-mincut of sum_i E_i(x_i) + sum_k E_k(x_u, x_v), unary
 * (n x 2: E(0), E(1)), pair (m x 4: E(00), E(01), E(10), E(11)), Energy::
 * add_term1 / add_term2 (energy.h:204-245); seg[i] = 1 iff SINK.
 * labeling: labeling() itself as the engine runs it -- squared residuals r2,
 * squared truncated threshold sqt, lambda, the grid over n points of `dims`
 * row-major coordinates (cell_number 0: no grid); seg[i] = 1 iff inlier. */
int gcr_host_grid_edges(const double* points, size_t n, int dims, const double* cell_size, uint64_t cell_number,
                        uint32_t* edges_out, size_t cap, size_t* m_out);
int gcr_host_bk_energy(size_t n, const double* unary, const uint32_t* edges, const double* pair, size_t m,
                       uint8_t* seg);
int gcr_host_labeling(const double* r2, size_t n, double sqt, double lambda, const double* points, int dims,
                      const double* cell_size, uint64_t cell_number, uint8_t* seg);
/* host-only: findWeightedMode (two_sift.hpp:354-394) as the fits use it */
double gcr_host_weighted_mode(const double* angles, const double* weights, size_t n, double bin_width);
/* host-only (no GPU): deterministic math and sampler used on both sides */
double gcr_host_log(double x);
double gcr_host_pow_m3(double t);
double gcr_host_atan2(double y, double x);
/* host-only: the op of gcr_debug_math below on one operand pair (ops 0-6,
 * 8-11; the host twin of each device primitive) */
double gcr_host_math(int op, double a, double b);
int gcr_host_sample(uint64_t seed, uint64_t index, uint32_t sub, uint32_t stream, uint32_t cls, uint64_t n,
                    uint32_t m, uint32_t* out);
/* host-only: PROSAC's growth table (csrc/prosac.h) of n rows, minimal sample
 * m <= 32 and convergence length 1 .. 2^40: g_out[0 .. n], the entries below
 * m are 0 */
int gcr_host_prosac_growth(size_t n, uint32_t m, uint64_t convergence, uint64_t* g_out);
/* host-only: the pool size n(slot + 1) of a slot by the flat search over that
 * table; *pool_out = 0 in the uniform phase (slot >= g[n]) */
int gcr_host_prosac_pool(size_t n, uint32_t m, uint64_t convergence, uint64_t slot, uint32_t* pool_out);
/* host-only: one PROSAC sample, the generators' function: attempt `sub` of
 * slot `index` (main stream, class 0), m indices in out */
int gcr_host_sample_prosac(uint64_t seed, uint64_t index, uint32_t sub, size_t n, uint32_t m, uint64_t convergence,
                           uint32_t* out);
/* host-only: the PROSAC stop's tables (csrc/prosac_stop.h) for n rows, minimal
 * sample m, that growth table and `confidence`: imin_out[0 .. n] and
 * qmin_out[0 .. n], the entries below m are 0 */
int gcr_host_prosac_stop_tables(size_t n, uint32_t m, uint64_t convergence, double confidence, uint32_t* imin_out,
                                double* qmin_out);
/* host-only: the PROSAC stop's choice, the kernel's host twin: (I*, n*) of the
 * inlier mask (n bytes in row order, nonzero = inlier) under those tables */
int gcr_host_prosac_stop(const uint8_t* mask, size_t n, uint32_t m, const uint32_t* imin, const double* qmin,
                         uint32_t* best_i, uint32_t* best_n);
/* host-only: the PROSAC stop itself, the function the engine calls: the
 * reference's iteration bound with ratio best_i / best_n for a minimal sample
 * of m at `confidence` (UINT64_MAX where the reference's guard returns it).
 * best_n == 0 or best_i > best_n: GCR_EINVAL */
int gcr_host_prosac_stop_number(uint32_t best_i, uint32_t best_n, uint32_t m, double confidence, uint64_t* out);
/* host-only: NAPSAC's layers (csrc/napsac.h) of n rows (x1, y1, x2, y2) over
 * extent {w1, h1, w2, h2}: members_out[l * n ..] is grid layer l's member list
 * (l = 0..3: 16, 8, 4, 2 cells per axis; cells in key order, rows ascending
 * inside), start / count / pos_out[l * n + i] row i's cell in that layer */
int gcr_host_napsac_layers(const double* rows, size_t n, const double extent[4], uint32_t* members_out,
                           uint32_t* start_out, uint32_t* count_out, uint32_t* pos_out);
/* host-only: one NAPSAC sample, the generators' function: attempt `sub` of
 * slot `index` (main stream, class 0) with local length 1 .. 2^40, m <= 32
 * indices in out; gcr_host_samples_napsac: attempt `sub` of nslots slots from
 * slot0 over one set of layers (out: m per slot, all-ones where the draw
 * budget ran out) */
int gcr_host_sample_napsac(uint64_t seed, uint64_t index, uint32_t sub, const double* rows, size_t n, uint32_t m,
                           const double extent[4], uint64_t local_iterations, uint32_t* out);
int gcr_host_samples_napsac(uint64_t seed, uint64_t slot0, uint32_t nslots, uint32_t sub, const double* rows, size_t n,
                            uint32_t m, const double extent[4], uint64_t local_iterations, uint32_t* out);
/* host-only: the host twin of a correspondence generator under NAPSAC
 * sampling, for all five solvers (gcr_host_generate_e / _g / _s with the
 * NAPSAC sampler, and the same for the 4-point homography and the 7-point
 * fundamental matrix).  correspondences: the rows the solver reads (K-normalised
 * for the essential solvers); pixels: the rows the layers lie over (NULL: the
 * correspondences themselves); sift, G1 / G2: for the solver that takes them,
 * NULL for the others.  inc_out / models_out as gcr_debug_generate_h's. */
int gcr_host_generate_napsac(int solver, const double* correspondences, const double* pixels, const double* sift,
                             const double* G1, const double* G2, size_t n, const double extent[4],
                             uint64_t local_iterations, uint64_t seed, uint64_t slot0, uint32_t nslots, int threads,
                             uint8_t* inc_out, double* models_out);
/* host-only: the check gcr_problem_set_probabilities makes of its weights for
 * a minimal sample of m (GCR_OK, or GCR_EINVAL with a message) */
int gcr_host_check_probabilities(const double* probabilities, size_t n, uint32_t m);
/* host-only: one guided sample (csrc/guided.h) from raw weights: m <= 32
 * distinct indices in draw order; the weights are checked as
 * gcr_problem_set_probabilities checks them, with m as the minimal size */
int gcr_host_sample_guided(uint64_t seed, uint64_t index, uint32_t sub, uint32_t stream, uint32_t cls,
                           const double* probabilities, size_t n, uint32_t m, uint32_t* out);
/* host-only: the index one 64-bit word of the stream selects (the generators'
 * two-level search, guided_index), weights checked as above: the draws no
 * seed reaches in a test's time, such as word = 2^64 - 1 */
int gcr_host_guided_index(const double* probabilities, size_t n, uint32_t m, uint64_t word, uint32_t* out);
/* host-only: the guided stop's quanta (csrc/guided_stop.h) of raw weights,
 * checked as gcr_problem_set_probabilities checks them with m as the minimal
 * size: q_out[i] = (uint64_t)(w[i] / total * 2^(52 - bit_length(n))), *Q_out
 * their sum (< 2^52; 0 is possible for n >= 2^26 only) */
int gcr_host_guided_quanta(const double* probabilities, size_t n, uint32_t m, uint64_t* q_out, uint64_t* Q_out);
/* host-only: the guided stop itself, the function the engine calls: the
 * reference's iteration bound with ratio mass / Q for a minimal sample of m
 * at `confidence` (UINT64_MAX where the reference's guard returns it).
 * Q == 0, mass > Q or Q >= 2^52: GCR_EINVAL */
int gcr_host_guided_iterations(uint64_t mass, uint64_t Q, uint32_t m, double confidence, uint64_t* out);
/* device evaluation of the same primitives over arrays (GPU parity tests):
 * op 0 log(a), 1 pow_m3(a), 2 atan2(a, b), 3 a / b, 4 sqrt(a),
 * 5 clip_angle_small(a), 6 clip_angle(a), 8 round 3's log (dm_log_fd),
 * 9 / 10 sin / cos of a (dm_sincos), 11 atan(a / b) for 0 <= a <= b
 * (atan_ratio, the orientation value's);
 * op 7 (n >= 2): out[0] = the block-parallel exact in-order sum of a[0, n)
 * (k_lo_chain's fold), out[1] = the same sum by a sequential loop;
 * op 12 (7 <= n <= 8192, split h = b[0]): out[0..2] = the three chains of
 * k_lo_chain's two-class fold (a[0, h) from +0, a[h, n) from +0, a[h, n)
 * from out[0]), out[3..5] = the same by sequential loops, out[6] = cycles */
int gcr_debug_math(gcr_ctx* ctx, int op, const double* a, const double* b, size_t n, double* out);
/* perspective_warp's resampling (examples/utils.py:92-123, cv2.warpPerspective
 * with INTER_LINEAR): dst pixel (x, y) <- bilinear sample of src at
 * M (x, y, 1)^T / w, M = the dst -> src map (the inverse of the translated
 * homography), row-major.  Host buffers, channels interleaved, 1 <= channels
 * <= 4; dtype 0 = uint8 (rounded, saturated), 1 = float32.  border_mode 0 =
 * constant border_value[c], 1 = replicate the nearest edge pixel. */
int gcr_warp_perspective(gcr_ctx* ctx, const void* src, int src_h, int src_w, int channels, int dtype,
                         const double M[9], int border_mode, const double border_value[4], void* dst, int dst_h,
                         int dst_w);
/* Exact 2-nearest-neighbour matching of uint8 descriptors (csrc/match.h is
 * the definition, csrc/match.hip the int8 matrix-core kernels).  d1 is n1 x
 * dim, d2 is n2 x dim, row-major host buffers; dim is a multiple of 32 in
 * 32..512; 1 <= n1, n2 <= 2^24.  d(i, j) = sum_k (d1[i,k] - d2[j,k])^2.  For
 * every row i of d1 the neighbours are ordered by (d(i, j), j) -- on a tie the
 * lower index is nearer -- and idx_out / dist_out take the first, idx2_out /
 * dist2_out the second element of that order (0xFFFFFFFF both for n2 == 1);
 * n1 values each.  The device result equals gcr_host_match_descriptors' bit
 * for bit.  A NULL buffer, a bad n1, n2 or dim is GCR_EINVAL with a message
 * naming the argument, before any GPU work (so also with a NULL context).
 * GCR_MATCH_SPLIT=k in the environment pins the number of column splits
 * (tests).  ms_kernel_out may be NULL: HIP-event time of the kernels. */
int gcr_match_descriptors(gcr_ctx* ctx, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2, uint32_t dim,
                          uint32_t* idx_out, uint32_t* dist_out, uint32_t* idx2_out, uint32_t* dist2_out,
                          double* ms_kernel_out);
/* host-only: the same by plain loops; `threads` (clamped to 1..64) splits the
 * rows of d1 only and does not change the result */
int gcr_host_match_descriptors(const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2, uint32_t dim, int threads,
                               uint32_t* idx_out, uint32_t* dist_out, uint32_t* idx2_out, uint32_t* dist2_out);
/* Guided matching (csrc/match_geo.h is the definition): the same 2-nearest-
 * neighbour search among the pairs a two-view model admits.  p1 (n1 x 2) and
 * p2 (n2 x 2) are the keypoint positions, row-major doubles (x, y); kind is
 * GCR_SOLVER_HOMOGRAPHY4 (squared transfer error of p1 -> p2 under the
 * homography `model`) or GCR_SOLVER_FUNDAMENTAL7 (squared Sampson distance
 * under the fundamental matrix `model`), the estimators' own residuals;
 * model is 9 doubles, row-major.  The pair (i, j) of row i of image 1 and row
 * j of image 2 is admissible iff its residual <= sq_threshold in fp64 (a NaN
 * residual never is; sq_threshold = +inf admits every other pair).
 * reverse = 0: for every i the first two admissible j in the order
 * (d(i, j), j), n1 values per output.  reverse = 1: for every j the first two
 * admissible i in the order (d(i, j), i), n2 values per output.  0xFFFFFFFF in
 * idx_out and dist_out where a row has no admissible candidate, in idx2_out
 * and dist2_out where it has one.  The device result equals
 * gcr_host_match_descriptors_guided's bit for bit.  Errors as
 * gcr_match_descriptors, and: NULL p1, p2 or model, another kind, a NaN or
 * negative sq_threshold, a non-finite model entry, reverse not 0 or 1. */
int gcr_match_descriptors_guided(gcr_ctx* ctx, const uint8_t* d1, size_t n1, const double* p1, const uint8_t* d2,
                                 size_t n2, const double* p2, uint32_t dim, int kind, const double* model,
                                 double sq_threshold, int reverse, uint32_t* idx_out, uint32_t* dist_out,
                                 uint32_t* idx2_out, uint32_t* dist2_out, double* ms_kernel_out);
/* host-only: the same by plain loops; `threads` (clamped to 1..64) splits the
 * result rows only and does not change the result */
int gcr_host_match_descriptors_guided(const uint8_t* d1, size_t n1, const double* p1, const uint8_t* d2, size_t n2,
                                      const double* p2, uint32_t dim, int kind, const double* model,
                                      double sq_threshold, int reverse, int threads, uint32_t* idx_out,
                                      uint32_t* dist_out, uint32_t* idx2_out, uint32_t* dist2_out);
/* the matcher kernels' tiling, for tests at its edges: out[0] = rows of d1 per
 * workgroup, out[1] = rows of d2 (columns) per step, out[2] = the least
 * columns per split the planner chooses */
void gcr_match_tiling(uint32_t out[3]);

/* Resident descriptor sets (csrc/match_sets.h): one image's descriptors on the
 * device, uploaded once with their norms and, optionally, the keypoint
 * positions.  Two sets are matched entirely on the device: the forward and
 * (mutual) the reverse search by the kernels of gcr_match_descriptors /
 * gcr_match_descriptors_guided, then csrc/match_select.h's rule -- the ratio
 * test, the distance cap, the mutual check, the ratios -- and an ordered
 * compaction of the kept rows; one synchronisation and one download end the
 * call.  The results are what the Python front end (features.match_descriptors,
 * features.match_descriptors_guided) computes from the array entries' outputs,
 * bit for bit.  What a call needs beyond the sets lives in a workspace of the
 * context that grows when a call needs more and is freed with the context: a
 * call whose shapes fit allocates nothing. */
typedef struct gcr_descriptors gcr_descriptors;

typedef struct gcr_match_options {
    int has_ratio;             /* 0: no ratio test */
    double rr;                 /* ratio * ratio, finite and > 0 */
    int mutual;                /* 0 or 1: keep (i, j) only if i is j's first neighbour too */
    int has_max_distance;      /* guided entries only; 0: no cap */
    double max_distance;       /* keep only dist <= max_distance; >= 0 */
} gcr_match_options;

/* d is n x dim uint8 under gcr_match_descriptors' ranges; positions is NULL or
 * n x 2 finite doubles (x, y).  A NULL argument, a bad n or dim, a non-finite
 * position: GCR_EINVAL naming the argument, before any GPU work.  The set
 * belongs to ctx and must be destroyed before it. */
int gcr_descriptors_create(gcr_ctx* ctx, const uint8_t* d, size_t n, uint32_t dim, const double* positions,
                           gcr_descriptors** out);
void gcr_descriptors_destroy(gcr_descriptors* set);     /* safe on NULL */
int gcr_descriptors_info(const gcr_descriptors* set, size_t* n_out, uint32_t* dim_out, int* has_positions_out);
/* The rows of `a` matched against `b` (which may be `a`).  matches_out takes
 * cap x 2 values, the pairs (i, j) in ascending i, ratios_out cap doubles,
 * sqrt(dist / dist2) or 1.0; *m_out their count.  cap must be at least a's row
 * count: nothing is ever truncated.  ms_kernel_out may be NULL; else FOUR
 * doubles of HIP-event times in ms: all kernels, the forward search, the
 * reverse search, the select launches.  GCR_EINVAL naming the argument for a
 * NULL argument, a set of another context, sets of different dim, a bad option. */
int gcr_match_sets(gcr_ctx* ctx, const gcr_descriptors* a, const gcr_descriptors* b, const gcr_match_options* opt,
                   uint32_t* matches_out, double* ratios_out, size_t cap, size_t* m_out, double* ms_kernel_out);
/* The same among the pairs `model` admits (kind, model, sq_threshold as
 * gcr_match_descriptors_guided checks them); both sets need positions.  A row
 * without an admissible candidate gives no match; one with a single candidate
 * passes the ratio test. */
int gcr_match_sets_guided(gcr_ctx* ctx, const gcr_descriptors* a, const gcr_descriptors* b, int kind,
                          const double* model, double sq_threshold, const gcr_match_options* opt,
                          uint32_t* matches_out, double* ratios_out, size_t cap, size_t* m_out,
                          double* ms_kernel_out);
/* gcr_match_sets over many pairs in one call: pairs is npairs x 2 indices into
 * sets (first the row side); every pair is queued, then one synchronisation
 * and one download.  offsets (npairs + 1, ascending) places pair p's rows at
 * matches_out + 2 * offsets[p] and ratios_out + offsets[p]; offsets[p + 1] -
 * offsets[p] must be at least the row count of the pair's first set.  m_out
 * takes npairs counts.  ms_kernel_out may be NULL; else ONE double, all
 * kernels.  npairs == 0 is valid and does nothing. */
int gcr_match_set_pairs(gcr_ctx* ctx, const gcr_descriptors* const* sets, size_t nsets, const uint32_t* pairs,
                        size_t npairs, const gcr_match_options* opt, uint32_t* matches_out, double* ratios_out,
                        const size_t* offsets, size_t* m_out, double* ms_kernel_out);
/* Exact k-nearest-neighbour search (csrc/match_knn.h is the definition,
 * csrc/match_knn.hip the kernels): gcr_match_descriptors' arguments, ranges,
 * distance and order, and 1 <= k <= 8.  idx_out / dist_out are n1 x k,
 * row-major: row i holds the first k elements of the order (d(i, j), j), and
 * 0xFFFFFFFF in both from position n2 on where n2 < k.  For k = 2 the two
 * columns are gcr_match_descriptors' idx / idx2 and dist / dist2.  The device
 * result equals gcr_host_knn_descriptors' bit for bit, under every
 * GCR_MATCH_SPLIT.  A NULL buffer, a bad n1, n2, dim or k is GCR_EINVAL with a
 * message naming the argument, before any GPU work.  ms_kernel_out may be
 * NULL: HIP-event time of the kernels. */
int gcr_knn_descriptors(gcr_ctx* ctx, const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2, uint32_t dim,
                        uint32_t k, uint32_t* idx_out, uint32_t* dist_out, double* ms_kernel_out);
/* host-only: the same by plain loops; `threads` (clamped to 1..64) splits the
 * rows of d1 only and does not change the result */
int gcr_host_knn_descriptors(const uint8_t* d1, size_t n1, const uint8_t* d2, size_t n2, uint32_t dim, uint32_t k,
                             int threads, uint32_t* idx_out, uint32_t* dist_out);
/* gcr_knn_descriptors on two resident sets (b may be a): the rows of `a`
 * against `b`, idx_out / dist_out rows(a) x k.  The sets' buffers and norms
 * and the context's matching workspace; one synchronisation and one download.
 * ms_kernel_out may be NULL; else ONE double.  GCR_EINVAL naming the argument
 * for a NULL argument, a bad k, a set of another context, sets of different dim. */
int gcr_knn_sets(gcr_ctx* ctx, const gcr_descriptors* a, const gcr_descriptors* b, uint32_t k, uint32_t* idx_out,
                 uint32_t* dist_out, double* ms_kernel_out);
/* host-only: csrc/match_select.h's rule by plain loops on a search's results
 * (n rows).  back is NULL (no mutual check) or the reverse search's idx (nb
 * values).  guided selects the guided variant of the rule. */
int gcr_host_match_select(const uint32_t* idx, const uint32_t* dist, const uint32_t* idx2, const uint32_t* dist2,
                          size_t n, const uint32_t* back, size_t nb, int guided, const gcr_match_options* opt,
                          uint32_t* matches_out, double* ratios_out, size_t cap, size_t* m_out);
/* the select kernels' tiling, for tests at its edges: out[0] = rows per workgroup */
void gcr_match_select_tiling(uint32_t out[1]);
/* out[0] = device allocations made so far for ctx's matching workspace (a set's
 * own buffers are not counted), out[1] = the workspace's device bytes held now */
int gcr_debug_match_workspace(gcr_ctx* ctx, uint64_t out[2]);
/* measurement (bench.py): achievable HBM bandwidth of the device, GB/s of
 * read + write traffic of a streaming device-to-device copy of `bytes` bytes,
 * best of `iters` timed copies of each of two variants, plain and nontemporal
 * (no reference counterpart) */
int gcr_measure_hbm(gcr_ctx* ctx, size_t bytes, int iters, double* gbps_out);

#ifdef __cplusplus
}
#endif

#endif /* GCR_H_ */
