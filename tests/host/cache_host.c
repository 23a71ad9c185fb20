/* tests/host/cache_host.c -- TEST INFRASTRUCTURE.  Host build (gcc) of the conversions the device kernels k_cache_load / k_cache_store run
 * (ssdnerf_amd/csrc/cache_cvt.h), over arrays of bit patterns. */
#include <stddef.h>
#include "../../ssdnerf_amd/csrc/cache_cvt.h"

void f32_to_f16_clamped(const uint32_t* x, uint16_t* y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = sscc_f32_to_f16_clamped(x[i]); }
void f32_to_bf16_clamped(const uint32_t* x, uint16_t* y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = sscc_f32_to_bf16_clamped(x[i]); }
void f16_to_f32(const uint16_t* x, uint32_t* y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = sscc_f16_to_f32(x[i]); }
void bf16_to_f32(const uint16_t* x, uint32_t* y, size_t n) { for (size_t i = 0; i < n; ++i) y[i] = sscc_bf16_to_f32(x[i]); }
