/*
 * slamgpu_pnpsolver.h -- C ABI of the relocalisation's RANSAC EPnP solver (libslamgpu.so), drop-in
 * for the arithmetic of (paths relative to the reference repository root)
 *   PnPsolver::iterate / Refine / compute_pose / CheckInliers      src/solvers/pnp_solver.cpp:118-903
 * as Tracker::Relocalization drives it (src/core/tracker.cpp:826-991): step 2 of the chain
 * SearchByBoW -> PnPsolver -> PoseOptimization -> SearchByProjection.
 *
 * The hypotheses of a candidate do not depend on one another and Refine() is a pure function of
 * the running best's mask, so one call evaluates the WHOLE schedule of every candidate: for
 * iteration k of job j the EPnP pose of its four-point sample (mRi, mti as float), the inlier
 * mask (mvbInliersi), its count (mnInliersi) and the iteration that holds the running best after
 * k; for every iteration b that became a best, Refine() of its inlier set (pose, mask, count);
 * and the ascending list of iterations at which the reference's iterate() would return
 * mRefinedTcw. The sequential part of iterate() / find() -- bNoMore, the iterations carried across
 * calls, the `||` of the loop condition -- is replayed on the host from those
 * (slamgpu_adapters.hpp: PnPSolverCore).
 *
 * The library takes no position on the random generator: the caller passes, per iteration, the
 * four values DUtils::Random::RandomInt returned (randi, :146), in [0, N-1], [0, N-2], [0, N-3]
 * and [0, N-4]; the device resolves them to correspondence indices as the swap-and-pop of
 * :148-153 does. mRansacMinSet is fixed at 4 (the reference's only caller). min_inliers is the
 * effective mRansacMinInliers after :87-92 and n_its the schedule length: the effective
 * mRansacMaxIts of :105, or more when iterate() runs past it (pnp_ransac_parameters in
 * slamgpu_adapters.hpp computes both with the reference's host expression).
 *
 * A correspondence is its map point's world position (mvP3Dw), the undistorted keypoint (mvP2D)
 * and the keypoint's octave. sigma2[nlevels] is the frame's level_sigma_sq (NOT the inverse); the
 * threshold of :109 is sigma2[octave] * th2 in float. A correspondence whose octave is outside
 * [0, nlevels) is never an inlier. K = fx, fy, cx, cy; they are widened to double as the
 * reference's fu, fv, uc, vc are.
 *
 * Arithmetic: DESIGN.md "RANSAC EPnP solver". Four-point EPnP is decided by rounding noise in the
 * null space of MtM, so the contract is this project's own CPU restatement
 * (tests/pnpsolver_ref.c), matched bit for bit, not OpenCV's cvSVD. Degenerate samples (coplanar,
 * collinear or repeated points, Zc = 0) propagate inf / NaN by IEEE rules; a NaN error is not an
 * inlier.
 *
 * Conventions as slamgpu_sim3solver.h: POD types, caller-owned buffers, 0 or a negative
 * SLAMGPU_E* code with the message in slamgpu_pnpsolver_last_error() (per thread). The
 * synchronous call takes host pointers and stages through the calling thread's device buffer;
 * the *_device call takes device pointers and a hipStream_t, never allocates and returns without
 * synchronising. K and sigma2 are host pointers in both.
 */
#ifndef SLAMGPU_PNPSOLVER_H_
#define SLAMGPU_PNPSOLVER_H_

#include <stddef.h>
#include <stdint.h>

#include "slamgpu_optimizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest schedule of a job: the reference's default maxIterations (300) and room for the
 * iterations iterate() runs past mRansacMaxIts (the `||` of :135). */
#define SLAMGPU_PNP_RANSAC_MAX_ITS 512
/* Largest correspondence count of a job. */
#define SLAMGPU_PNP_MAX_MATCHES 4096

/* One correspondence: mvP3Dw[i], mvP2D[i], the octave mvSigma2[i] was looked up with. 24 bytes. */
typedef struct {
  float xw[3];
  float u, v;
  int32_t octave;
} slamgpu_pnp_match;

/* One candidate keyframe. Its correspondences are d_matches[match_begin .. match_begin + n) and
 * its draws d_draws[draw_begin .. draw_begin + 4 n_its), four per iteration. 24 bytes. */
typedef struct {
  int32_t match_begin, n;     /* correspondences, N of the reference              */
  int32_t draw_begin, n_its;  /* schedule length                                  */
  int32_t min_inliers;        /* the effective mRansacMinInliers (:87-92), >= 4   */
  int32_t pad;
} slamgpu_pnp_ransac_job;

/* Iteration k of a job: mRi (row-major) and mti converted to float, mnInliersi, and the iteration
 * that holds the running best after k (-1: none reached min_inliers yet). A row of `refined`
 * uses the same record: best = its own index, or n_inliers = best = -1 and a zero pose for an
 * iteration that never became a best. 64 bytes. */
typedef struct {
  float Rcw[9], tcw[3];
  int32_t n_inliers, best;
  int32_t pad[2];
} slamgpu_pnp_hyp;

/* Mask words per hypothesis for correspondence counts up to max_n. */
#define SLAMGPU_PNP_MASK_WORDS(max_n) (((max_n) + 63) / 64)

/* Batched, asynchronous on `stream`. max_n >= every job's n (<= SLAMGPU_PNP_MAX_MATCHES) and
 * max_its >= every job's n_its (<= SLAMGPU_PNP_RANSAC_MAX_ITS) size the output rows:
 *   d_hyp[job][max_its], d_inlier_bits[job][max_its][words], words = SLAMGPU_PNP_MASK_WORDS(max_n)
 *     (bit i of word i / 64 = mvbInliersi[i]; all `words` words are written, tail bits 0),
 *   d_refined[job][max_its], d_refined_bits[job][max_its][words]: Refine() of the best set at
 *     iteration b (mRefinedTcw's R and t, mnRefinedInliers, mvbRefinedInliers),
 *   d_events[job][max_its], d_n_events[job].
 * Job j writes rows k < n_its only, events[j][0 .. n_events[j]) = the ascending k with
 * n_k >= min_inliers and refined[best_k].n_inliers > min_inliers (:162-189), and n_events[j].
 * n_events[j] = -1, and nothing else of the job is written, when its ranges leave the arrays,
 * n < 4, n > max_n, n_its is outside [1, max_its], min_inliers < 4 or a draw is out of its range.
 * No scratch is used. */
int slamgpu_pnp_ransac_device(const float K[4], const float* sigma2, int nlevels, float th2,
                              const slamgpu_pnp_match* d_matches, int n_matches_total,
                              const int32_t* d_draws, int n_draws_total,
                              const slamgpu_pnp_ransac_job* d_jobs, int n_jobs, int max_n,
                              int max_its, slamgpu_pnp_hyp* d_hyp, uint64_t* d_inlier_bits,
                              slamgpu_pnp_hyp* d_refined, uint64_t* d_refined_bits,
                              int32_t* d_events, int32_t* d_n_events, void* stream);

/* One job on host pointers: matches[n], draws[4 n_its]; hyp[n_its], inlier_bits[n_its][words],
 * refined[n_its], refined_bits[n_its][words] with words = SLAMGPU_PNP_MASK_WORDS(n),
 * events[n_its], *n_events. Synchronous. A draw out of range is SLAMGPU_EINVAL. */
int slamgpu_pnp_ransac(const float K[4], const float* sigma2, int nlevels, float th2,
                       const slamgpu_pnp_match* matches, int n, const int32_t* draws, int n_its,
                       int min_inliers, slamgpu_pnp_hyp* hyp, uint64_t* inlier_bits,
                       slamgpu_pnp_hyp* refined, uint64_t* refined_bits, int32_t* events,
                       int* n_events);

const char* slamgpu_pnpsolver_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAMGPU_PNPSOLVER_H_ */
