// ssdnerf_amd/csrc/adam_math.h -- one Adam step of one element, in fp32.
//
// The reference's optimizer: torch.optim.Adam with amsgrad=False, maximize=False, in its non-capturable single-tensor form
// (configs: optimizer=dict(type='Adam', lr=..., weight_decay=0.); one optimizer per scene code, lib/models/autodecoders/base_nerf.py
// build_optimizer).  Per element, with the host scalars of the step that is being taken:
//     g <- g + wd p                      only when wd != 0 (L2 regularisation folded into the gradient, NOT decoupled decay)
//     m <- m + (g - m) (1 - beta1)       torch's lerp at a weight below 0.5
//     v <- v beta2 + (1 - beta2) g g
//     p <- p - step_size m / (sqrt(v) / bc2_sqrt + eps),   step_size = lr / (1 - beta1^step),  bc2_sqrt = sqrt(1 - beta2^step)
// The host forms step_size, bc2_sqrt, 1 - beta1 and 1 - beta2 in double and passes them as float, as torch does with its Python scalars.
// Every operation is one IEEE fp32 operation (correctly rounded sqrt and division, no contraction: the library and the CPU harness are
// both built with -ffp-contract=off), so NaN and Inf gradients propagate exactly as they do through torch's kernels.
// Plain C: compiled by hipcc into k_adam_multi (adam.hip) and by gcc into the CPU test's harness (tests/host/adam_host.c).
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define SSDA_FN __device__ __forceinline__
#else
#define SSDA_FN static inline
#endif

// launch-wide scalars as the kernel receives them
typedef struct ssda_hyper {
    float beta2;             // (float)beta2
    float one_minus_beta1;   // (float)(1 - beta1)
    float one_minus_beta2;   // (float)(1 - beta2)
    float eps;
} ssda_hyper;

static inline ssda_hyper ssda_make_hyper(double beta1, double beta2, double eps) {
    ssda_hyper h;
    h.beta2 = (float)beta2;
    h.one_minus_beta1 = (float)(1.0 - beta1);
    h.one_minus_beta2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    return h;
}

// updates *p, *m, *v from the gradient g
SSDA_FN void ssda_step(float* p, float g, float* m, float* v, ssda_hyper h, float step_size, float bc2_sqrt, float weight_decay) {
    const float p0 = *p;
    if (weight_decay != 0.0f) g = g + weight_decay * p0;
    const float m1 = *m + (g - *m) * h.one_minus_beta1;
    const float v1 = *v * h.beta2 + h.one_minus_beta2 * g * g;
    const float denom = sqrtf(v1) / bc2_sqrt + h.eps;
    *m = m1;
    *v = v1;
    *p = p0 - step_size * (m1 / denom);
}
