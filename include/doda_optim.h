/*
 * doda_optim.h — companion C ABI of libdoda_hip.so: the optimizer step of the reference's three OPTIMIZATION.optim values (sgd, adam,
 * adamw: util/common_utils.py:196-215) with OPTIMIZATION.clip_grad (tool/train.py:100-104: clip_grad_norm_(parameters, 10) before
 * every step) folded in — one launch for all parameter tensors without the clip, two with it.
 *
 * Same conventions as doda_hip.h (whose error codes and doda_strerror these entry points use): extern "C", plain device pointers +
 * sizes, an explicit HIP stream, an int status.  Nothing here allocates device memory or synchronises; argument errors come back as
 * statuses without a launch.  The core header's surface (ABI 12, doda_sgd_multi included) and the other companions are unchanged;
 * this header carries its own version, DODA_OPTIM_ABI_VERSION, and the same library exports all of them.
 *
 * The update.  Hyper-parameters are doubles, parameters / gradients / state fp32; a mixed product is formed in double and rounded
 * once, as in torch's fused kernels (ATen/native/hip/fused_adam_utils.cuh adam_math, FusedSgdMathFunctor), whose arithmetic this is
 * term by term:
 *   DODA_OPTIM_SGD    g' = g (+ weight_decay * p);  buf = first_step ? g' : momentum * buf + (1 - dampening) * g';
 *                     g'' = nesterov ? g' + momentum * buf : buf  (g' when momentum == 0);  p -= lr * g''
 *                     (state1 = buf, may be NULL when momentum == 0; beta1 carries momentum, beta2 dampening)
 *   DODA_OPTIM_ADAM   g' = g + weight_decay * p;  m = beta1 * m + (1 - beta1) * g';  v = beta2 * v + (1 - beta2) * g' * g';
 *                     p -= (lr / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps)      (state1 = m, state2 = v)
 *   DODA_OPTIM_ADAMW  the same with g' = g and  p -= lr * weight_decay * p  first.
 * maximize negates the gradient that enters the update.  bias_correction1 = 1 - beta1^step and bias_correction2_sqrt =
 * sqrt(1 - beta2^step) are the caller's, per tensor (a tensor's step count is host state); the kernel uses them rounded to fp32.
 *
 * The clip (max_norm > 0).  A first launch sums the squares of all gradients: fp64 accumulation (an fp32 x fp32 product is exact in
 * fp64), one fp64 partial per workgroup written with a plain store, the grid capped at DODA_OPTIM_NORM_BLOCKS workgroups that stride
 * over the tiles.  There is no atomic and no last-block handshake: every workgroup of the update launch adds the partials in one fixed
 * order in its prologue, so all of them hold the same  norm = sqrt(sum)  and  coef = min(1, max_norm / (norm + 1e-6))  (fp64, rounded
 * to fp32 once — torch.nn.utils.clip_grad_norm_'s formula), bit for bit and run after run.  The gradient that enters the update is
 * g * coef (fp32), and it is STORED BACK: after the call g holds what clip_grad_norm_ would have left.  norm_out receives the norm as
 * fp32.  A non-finite sum gives a non-finite coef and non-finite parameters (clip_grad_norm_ with error_if_nonfinite=False).
 * With max_norm <= 0 nothing of this runs, g is only read and norm_out is not touched.
 */
#ifndef DODA_OPTIM_H
#define DODA_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#include "doda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DODA_OPTIM_ABI_VERSION 1

#define DODA_OPTIM_SGD 0
#define DODA_OPTIM_ADAM 1
#define DODA_OPTIM_ADAMW 2

#define DODA_OPTIM_TILE 2048          /* elements per workgroup of both launches */
#define DODA_OPTIM_NORM_BLOCKS 512    /* most workgroups (and fp64 partials) of the sum-of-squares launch */

typedef struct {
    float *p;
    float *g;                         /* written only under the clip */
    float *state1;                    /* sgd: momentum buffer (NULL when momentum == 0); adam / adamw: exp_avg */
    float *state2;                    /* adam / adamw: exp_avg_sq; sgd: unused */
    int64_t n;                        /* elements, 0 <= n < 2^31 */
    double bias_correction1;          /* adam / adamw */
    double bias_correction2_sqrt;     /* adam / adamw */
    int32_t first_step;               /* sgd: the momentum buffer holds no value yet */
    int32_t reserved;
} doda_optim_tensor;

typedef struct {
    double lr;
    double beta1;                     /* sgd: momentum */
    double beta2;                     /* sgd: dampening */
    double eps;                       /* adam / adamw */
    double weight_decay;
    int32_t nesterov;                 /* sgd */
    int32_t maximize;
} doda_optim_hyper;

int32_t doda_optim_abi_version(void);

/* Bytes of the device workspace of a step over n_tensors tensors (their descriptors and the fp64 partials); 0 for n_tensors <= 0. */
size_t doda_optim_workspace_bytes(int32_t n_tensors);

/* One step as described above.  tensors_h, hyper_h: HOST memory, read before the call returns.  norm_out: device fp32 scalar,
 * required when max_norm > 0.  ws: 16-byte aligned device memory of at least doda_optim_workspace_bytes(n_tensors) bytes
 * (DODA_ERR_WORKSPACE), owned by the call until the stream has passed it.  n_tensors == 0 is DODA_OK and launches nothing, as does a
 * list whose tensors are all empty.  DODA_ERR_INVALID: a null argument, n_tensors < 0, an unknown kind, a tensor with n outside
 * [0, 2^31), a tensor with n > 0 and no p or g or a missing state buffer (adam / adamw: state1 and state2; sgd with momentum:
 * state1) — an empty tensor may come without storage —, max_norm > 0 without norm_out, a misaligned ws. */
int doda_optim_step(const doda_optim_tensor *tensors_h, int32_t n_tensors, int32_t kind, const doda_optim_hyper *hyper_h,
                    double max_norm, float *norm_out, void *ws, size_t ws_bytes, doda_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DODA_OPTIM_H */
