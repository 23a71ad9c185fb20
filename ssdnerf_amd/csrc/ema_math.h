// ssdnerf_amd/csrc/ema_math.h -- the exponential moving average of one element, in fp32.
//
// The reference's hook (configs: custom_hooks[0], type='ExponentialMovingAverageHook', interp_mode='lerp'; mmgen 0.7.2) updates every entry of
// an EMA module's state dict from its source module with
//     lerp(a, b, momentum, momentum_nontrainable, trainable):  m = momentum if trainable else momentum_nontrainable;  return a + (b - a) * m
// where a is the SOURCE tensor and b the EMA tensor.  On fp32 tensors that is three eager kernels, each one IEEE operation per element:
//     ema <- fl32( src + fl32( fl32(ema - src) * m ) ),   m = (float)momentum
// Three separate roundings: no fused multiply-add and not the `lerp` identity (torch.lerp rounds differently; about 2 600 of 2^20 elements
// differ).  fp32 denormals are kept, NaN and Inf propagate as they do through the eager kernels ((inf - src) * 0 is NaN, not src).
// Plain C: compiled by hipcc into k_ema_multi (ema.hip), where the three operations are the explicitly rounded intrinsics, and by gcc with
// -ffp-contract=off into the CPU test's harness (tests/host/ema_host.c).
#pragma once

#ifdef __HIPCC__
#define SSDE_FN __device__ __forceinline__
#else
#define SSDE_FN static inline
#endif

// the new EMA value of one element
SSDE_FN float ssde_update(float ema, float src, float m) {
#ifdef __HIP_DEVICE_COMPILE__
    return __fadd_rn(src, __fmul_rn(__fsub_rn(ema, src), m));
#else
    const float d = ema - src;
    const float p = d * m;
    return src + p;
#endif
}
