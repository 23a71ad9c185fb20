/* tests/host/adam_host.c -- TEST INFRASTRUCTURE.  Host build (gcc, -ffp-contract=off) of the arithmetic the device kernel k_adam_multi runs
 * (ssdnerf_amd/csrc/adam_math.h): one Adam step of n elements in place, with the host scalars the C ABI takes. */
#include <stddef.h>
#include "../../ssdnerf_amd/csrc/adam_math.h"

void adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double beta1, double beta2, double eps,
               float step_size, float bc2_sqrt, float weight_decay) {
    const ssda_hyper h = ssda_make_hyper(beta1, beta2, eps);
    for (size_t i = 0; i < n; ++i) ssda_step(param + i, grad[i], exp_avg + i, exp_avg_sq + i, h, step_size, bc2_sqrt, weight_decay);
}
