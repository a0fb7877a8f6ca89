/*
 * slamgpu_sim3solver.h -- C ABI of the loop closer's RANSAC Sim3 solver (libslamgpu.so), drop-in
 * for the arithmetic of (paths relative to the reference repository root)
 *   Sim3Solver::iterate / ComputeSim3 / CheckInliers      src/solvers/sim3solver.cpp:142-368
 * as LoopCloser::ComputeSim3 drives it (src/core/loop_closer.cpp:299-422): step 2 of the chain
 * SearchByBoW -> Sim3Solver -> SearchBySim3 -> OptimizeSim3 -> SearchByProjection.
 *
 * The hypotheses of a candidate do not depend on one another, so one call evaluates the WHOLE
 * schedule of every candidate: for iteration k of job j the Horn transform of its three-point
 * sample (mR12i, mt12i, ms12i), the inlier mask (mvbInliersi) and its count (mnInliersi), and
 * the ascending list of iterations at which the reference's iterate() would return a transform.
 * The sequential part of iterate() / find() -- the running best, bNoMore, the iterations carried
 * across calls -- is replayed on the host from those (slamgpu_adapters.hpp: Sim3SolverCore).
 *
 * The library takes no position on the random generator: the caller passes, per iteration, the
 * three values DUtils::Random::RandomInt returned (randi, :171), in [0, N-1], [0, N-2] and
 * [0, N-3]; the device resolves them to correspondence indices as the swap-and-pop of :173-179
 * does. n_its is the effective mRansacMaxIts of :127-137 (sim3_ransac_iterations in
 * slamgpu_adapters.hpp computes it with the reference's host libm expression).
 *
 * Correspondences are slamgpu_sim3_match records as gather_optimize_sim3 fills them; the solver
 * reads x1c, x2c, octave1 and octave2 only (it compares projections of the camera-frame points,
 * mvP1im1 / mvP2im2 of :110-111, never keypoints). sigma2_1 / sigma2_2[nlevels] are the
 * keyframes' level_sigma_sq (NOT the inverse); the thresholds are the reference's
 * std::vector<size_t> entries: (float)(size_t)(9.210 * (double)sigma2[octave]), i.e. truncated
 * to an integer (9, 13, 19, 27, ... at scale factor 1.2). A correspondence whose octave is
 * outside [0, nlevels) is never an inlier.
 *
 * Arithmetic: DESIGN.md "RANSAC Sim3 solver". Degenerate samples (collinear or repeated points,
 * z = 0, den = 0) propagate inf / NaN by IEEE rules; a NaN error is not an inlier.
 *
 * Conventions as slamgpu_loopmatch.h: POD types, caller-owned buffers, 0 or a negative
 * SLAMGPU_E* code with the message in slamgpu_sim3solver_last_error() (per thread). The
 * synchronous call takes host pointers and stages through the calling thread's device buffer;
 * the *_device call takes device pointers and a hipStream_t, never allocates and returns without
 * synchronising. K1 / K2 / sigma2_* are host pointers in both.
 */
#ifndef SLAMGPU_SIM3SOLVER_H_
#define SLAMGPU_SIM3SOLVER_H_

#include <stddef.h>
#include <stdint.h>

#include "slamgpu_optimizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest iteration count of a job (the reference's default maxIterations). */
#define SLAMGPU_SIM3_RANSAC_MAX_ITS 300

/* One candidate keyframe. Its correspondences are d_matches[match_begin .. match_begin + n) and
 * its draws d_draws[draw_begin .. draw_begin + 3 n_its), three per iteration. 24 bytes. */
typedef struct {
  int32_t match_begin, n;      /* correspondences, N of the reference        */
  int32_t draw_begin, n_its;   /* n_its = the effective mRansacMaxIts (:137)  */
  int32_t min_inliers, fix_scale;
} slamgpu_sim3_ransac_job;

/* Iteration k of a job: mR12i (row-major), mt12i, ms12i, mnInliersi. 64 bytes. */
typedef struct {
  float R12[9], t12[3], s12;
  int32_t n_inliers;
  int32_t pad[2];
} slamgpu_sim3_hyp;

/* Mask words per hypothesis for correspondences counts up to max_n. */
#define SLAMGPU_SIM3_MASK_WORDS(max_n) (((max_n) + 63) / 64)

/* Batched, asynchronous on `stream`. max_n >= every job's n (<= SLAMGPU_SIM3_MAX_MATCHES) and
 * max_its >= every job's n_its (<= SLAMGPU_SIM3_RANSAC_MAX_ITS) size the output rows:
 *   d_hyp[job][max_its], d_inlier_bits[job][max_its][words], words = SLAMGPU_SIM3_MASK_WORDS(max_n)
 *     (bit i of word i / 64 = mvbInliersi[i]; all `words` words are written, tail bits 0),
 *   d_events[job][max_its], d_n_events[job].
 * Job j writes rows k < n_its only, events[j][0 .. n_events[j]) = the ascending k with
 * n_k >= max(n_0 .. n_{k-1}) and n_k > min_inliers (:186-195), and n_events[j]. n_events[j] = -1,
 * and nothing else of the job is written, when its ranges leave the arrays, n < 3, n > max_n,
 * n_its is outside [1, max_its] or a draw is out of its range. No scratch is used. */
int slamgpu_sim3_ransac_device(const float K1[4], const float K2[4], const float* sigma2_1,
                               const float* sigma2_2, int nlevels,
                               const slamgpu_sim3_match* d_matches, int n_matches_total,
                               const int32_t* d_draws, int n_draws_total,
                               const slamgpu_sim3_ransac_job* d_jobs, int n_jobs, int max_n,
                               int max_its, slamgpu_sim3_hyp* d_hyp, uint64_t* d_inlier_bits,
                               int32_t* d_events, int32_t* d_n_events, void* stream);

/* One job on host pointers: matches[n], draws[3 n_its]; hyp[n_its], inlier_bits[n_its][words]
 * with words = SLAMGPU_SIM3_MASK_WORDS(n), events[n_its], *n_events. Synchronous. A draw out of
 * range is SLAMGPU_EINVAL. */
int slamgpu_sim3_ransac(const float K1[4], const float K2[4], const float* sigma2_1,
                        const float* sigma2_2, int nlevels, const slamgpu_sim3_match* matches,
                        int n, const int32_t* draws, int n_its, int min_inliers, int fix_scale,
                        slamgpu_sim3_hyp* hyp, uint64_t* inlier_bits, int32_t* events,
                        int* n_events);

const char* slamgpu_sim3solver_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAMGPU_SIM3SOLVER_H_ */
