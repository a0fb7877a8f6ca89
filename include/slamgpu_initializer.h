/*
 * slamgpu_initializer.h -- C ABI of the monocular Initializer (libslamgpu.so), drop-in for the
 * arithmetic of (paths relative to the reference repository root)
 *   Initializer::Initialize / FindHomography / FindFundamental / ReconstructH / ReconstructF /
 *   CheckRT / Triangulate / DecomposeE / Normalize                src/util/initializer.cpp:22-944
 * as Tracker::MonocularInitialization drives it (src/core/tracker.cpp:297-343) on every frame
 * until a map exists. vMatches12 is OrbMatcher::SearchForInitialization's output: on the device,
 * slamgpu_search_for_initialization (slamgpu.h) on the frame slamgpu_frame_mono left in the context.
 *
 * The 2 x n_its hypotheses depend only on their draws, the best of a model is a prefix maximum
 * under strict >, and the 4 or 8 motion hypotheses of the chosen model do not depend on one
 * another, so ONE call evaluates all of it: per iteration and model the 3 x 3 matrix (H21i or
 * F21i), its score and its inlier mask; per job the best iteration of each model, SH, SF, RH and
 * the model the reference reconstructs from; per motion hypothesis R, t, CheckRT's nGood, its
 * vbGood mask, its vP3D and the cosine the parallax is taken from. What is sequential and small
 * stays on the host (slamgpu_adapters.hpp: InitializerCore): drawing the schedule, acos() of the
 * cosine and the thresholds of :495-565 / :693-735.
 *
 * The library takes no position on the random generator: the caller passes, per iteration, the
 * eight values DUtils::Random::RandomInt returned (:69), in [0, N-1-j] for j = 0..7; the device
 * resolves them to match indices as the swap-and-pop of :64-76 does.
 *
 * keys are the undistorted keypoint positions (x, y) of a frame; matches12[i] is the frame-2 key
 * of frame-1 key i or -1. K = fx, fy, cx, cy. N is the number of matches12 entries >= 0.
 *
 * Arithmetic: DESIGN.md "Monocular Initializer". Data is float as the reference's CV_32F Mats;
 * every SVD is the FP64 one-sided Jacobi of the EPnP solver's linear algebra contract, cv::Mat
 * products, inverses and determinants are this project's stated rule, and the contract is this
 * project's own CPU restatement (tests/initializer_ref.c), matched bit for bit, not OpenCV's
 * routines. inf and NaN propagate by IEEE rules; a NaN score never wins.
 *
 * Conventions as slamgpu_pnpsolver.h: POD types, caller-owned buffers, 0 or a negative SLAMGPU_E*
 * code with the message in slamgpu_initializer_last_error() (per thread). The synchronous call
 * takes host pointers and stages through the calling thread's device buffer; the *_device call
 * takes device pointers and a hipStream_t, never allocates and returns without synchronising.
 */
#ifndef SLAMGPU_INITIALIZER_H_
#define SLAMGPU_INITIALIZER_H_

#include <stddef.h>
#include <stdint.h>

#include "slamgpu_optimizer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest keypoint count of a frame. */
#define SLAMGPU_INIT_MAX_KEYS 8192
/* Largest schedule of a job (the reference's caller asks for 200). */
#define SLAMGPU_INIT_MAX_ITS 512
/* ReconstructH's eight motion hypotheses; ReconstructF uses the first four rows. */
#define SLAMGPU_INIT_MAX_MOTIONS 8
#define SLAMGPU_INIT_MODEL_H 0
#define SLAMGPU_INIT_MODEL_F 1

/* One pair of frames. Its frame-1 keys are d_keys1[key1_begin .. + n1), matches12 uses the same
 * range of d_matches12; frame 2 is d_keys2[key2_begin .. + n2); its draws are
 * d_draws[draw_begin .. + 8 n_its). 48 bytes. */
typedef struct {
  int32_t key1_begin, n1;
  int32_t key2_begin, n2;
  int32_t draw_begin, n_its;
  float K[4];  /* fx, fy, cx, cy */
  float sigma; /* mSigma */
  int32_t pad;
} slamgpu_init_job;

/* Iteration k of a model: H21i or F21i (row-major) and currentScore. 48 bytes. */
typedef struct {
  float M[9];
  float score;
  int32_t pad[2];
} slamgpu_init_hyp;

/* Per job. status 0, or -1 for a rejected job (nothing else of the job is written). best[m] is the
 * lowest iteration with the greatest score of model m among scores > 0, or -1 (then S = 0).
 * model = H when RH > 0.40. n_motions: 8 (H), 4 (F), or 0 for ReconstructH's early return (:601)
 * and for a chosen model without a best. norm: meanX, meanY, sX, sY of Normalize for frame 1, then
 * for frame 2. 80 bytes. */
typedef struct {
  int32_t status, n;
  int32_t best[2];
  float SH, SF, RH;
  int32_t model, n_motions;
  float norm[8];
  int32_t pad[3];
} slamgpu_init_result;

/* One motion hypothesis in the reference's order (ReconstructF: (R1,t) (R2,t) (R1,-t) (R2,-t);
 * ReconstructH: vR[i], vt[i]): CheckRT's return and the cosine at rank min(50, nGood - 1) of the
 * ascending vCosParallax (0 when nGood = 0; NaN sorts last). 64 bytes. */
typedef struct {
  float R[9], t[3];
  int32_t n_good;
  float cos_parallax;
  int32_t pad[2];
} slamgpu_init_motion;

#define SLAMGPU_INIT_MASK_WORDS(max_n1) (((max_n1) + 63) / 64)

/* Batched, asynchronous on `stream`. max_n1 >= every job's n1 (<= SLAMGPU_INIT_MAX_KEYS) and
 * max_its >= every job's n_its (<= SLAMGPU_INIT_MAX_ITS) size the output rows; words =
 * SLAMGPU_INIT_MASK_WORDS(max_n1):
 *   d_hyp[job][2][max_its], d_bits[job][2][max_its][words] (bit i = vbCurrentInliers[i] over the
 *     N matches; all `words` words are written, tail bits 0), rows k < n_its;
 *   d_result[job];
 *   d_pairs[job][max_n1][2]: mvMatches12 (first, second), rows < N;
 *   d_motion[job][8], d_good_bits[job][8][words] (vbGood over the n1 keys, all words written),
 *   d_p3d[job][8][max_n1][3] (vP3D, rows < n1, zero where CheckRT writes nothing): motions
 *     < n_motions only.
 * A job is rejected (status -1 and nothing else) when its ranges leave the arrays, n1 > max_n1,
 * n2 is outside [1, SLAMGPU_INIT_MAX_KEYS], n_its is outside [1, max_its], a matches12 entry is
 * outside [-1, n2), N < 8 or a draw is out of its range. No scratch is used. */
int slamgpu_init_ransac_device(const float* d_keys1, const int32_t* d_matches12, int n_keys1_total,
                               const float* d_keys2, int n_keys2_total, const int32_t* d_draws,
                               int n_draws_total, const slamgpu_init_job* d_jobs, int n_jobs,
                               int max_n1, int max_its, slamgpu_init_hyp* d_hyp, uint64_t* d_bits,
                               slamgpu_init_result* d_result, int32_t* d_pairs,
                               slamgpu_init_motion* d_motion, uint64_t* d_good_bits, float* d_p3d,
                               void* stream);

/* One job on host pointers, rows sized by n1 and n_its: keys1[n1][2], matches12[n1], keys2[n2][2],
 * draws[8 n_its]; hyp[2][n_its], bits[2][n_its][words], pairs[n1][2], motion[8],
 * good_bits[8][words], p3d[8][n1][3], words = SLAMGPU_INIT_MASK_WORDS(n1). Synchronous. A job the
 * device would reject is SLAMGPU_EINVAL (SLAMGPU_ECAP over a cap) and nothing is written. */
int slamgpu_init_ransac(const float* keys1, const int32_t* matches12, int n1, const float* keys2,
                        int n2, const float K[4], float sigma, const int32_t* draws, int n_its,
                        slamgpu_init_hyp* hyp, uint64_t* bits, slamgpu_init_result* result,
                        int32_t* pairs, slamgpu_init_motion* motion, uint64_t* good_bits,
                        float* p3d);

const char* slamgpu_initializer_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAMGPU_INITIALIZER_H_ */
