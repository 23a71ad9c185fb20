// tools/ubench/philox_ulp.hip -- the three library functions of the normal generator (csrc/philox.h: ssph_log, ssph_sqrt, ssph_sincos2pi), each over EVERY
// argument the generator can feed it: the 2^23 uniforms u = (m + 0.5) 2^-23.  The host side (tools/bench_sde.py --ulp) compares the four arrays with float64
// and writes the worst errors, in ulps of the exact result, into profiles/sde.json (device_function_ulp): the constants of tests/_philox_ref.normal_bounds.
// A property of the device library the build links, not of the kernels; the same flags as the library's sources so that the same functions are inlined.
// Build (tools/bench_sde.py does it on demand, with ssdnerf_amd.build.FLAGS): hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -shared philox_ulp.hip -o libphilox_ulp.so
#include <hip/hip_runtime.h>
#include "../../ssdnerf_amd/csrc/philox.h"

// m = first .. first + count - 1 (count a multiple of nothing in particular; one lane per argument): ln u, sqrt(-2 fl(ln u)), sin 2 pi u, cos 2 pi u
__global__ void k_philox_ulp(uint32_t first, uint32_t count, float* ln_u, float* root, float* sin_u, float* cos_u) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float u = ssph_uniform(first + i);
    const float l = ssph_log(u);
    float s, c;
    ssph_sincos2pi(u, &s, &c);
    ln_u[i] = l;
    root[i] = ssph_sqrt(-2.0f * l);
    sin_u[i] = s;
    cos_u[i] = c;
}

extern "C" int philox_ulp_eval(uint32_t first, uint32_t count, float* ln_u, float* root, float* sin_u, float* cos_u, void* stream) {
    if (count == 0) return 0;
    if (!ln_u || !root || !sin_u || !cos_u || (uint64_t)first + count > (1u << 23)) return 1;
    hipLaunchKernelGGL(k_philox_ulp, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream, first, count, ln_u, root, sin_u, cos_u);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
