/* tests/host/ema_host.c -- TEST INFRASTRUCTURE.  Host build (gcc, -ffp-contract=off) of the arithmetic the device kernel k_ema_multi runs
 * (ssdnerf_amd/csrc/ema_math.h): the EMA update of n elements in place. */
#include <stddef.h>
#include "../../ssdnerf_amd/csrc/ema_math.h"

void ema_update(float* ema, const float* src, size_t n, float m) {
    for (size_t i = 0; i < n; ++i) ema[i] = ssde_update(ema[i], src[i], m);
}
