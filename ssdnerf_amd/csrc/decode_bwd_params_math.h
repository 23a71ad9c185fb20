// ssdnerf_amd/csrc/decode_bwd_params_math.h -- gradient of the triplane decode w.r.t. the DECODER's parameters, per (sample, hidden unit).
//
// What autograd gets through the four nn.Linear layers when the rendering loss is differentiated with a trainable decoder (the closing iteration of every training
// step: lib/models/autodecoders/multiscene_nerf.py, loss_decoder + backward).  Notation of decode_bwd_math.h; one sample contributes
//
//   a_i  = dsa w_s,i silu'(h_i)           (density branch)
//   e_i  = dc_i silu'(u_i)                (colour branch; u_i = h_i + d_i, dc_i = sum_j dz_j Wc_ji)
//   dW1_ik += (a_i + e_i) f_k             db1_i += a_i + e_i
//   dWd_im += e_i SH_m                    dbd_i += e_i
//   dws_i  += dsa silu(h_i)               dbs   += dsa
//   dWc_ji += dz_j silu(u_i)              dbc_j += dz_j
//
// with dsa and dz_j from ssdb_heads (decode_bwd_math.h, colour form: the routine ssdb_mlp_backward starts from) and a_i + e_i formed as its dh_i: fma(dc_i, silu'(u_i), a_i).
// No gradient flows to positions or directions.
//
// The arithmetic is split where the kernel (decode_bwd_params.hip) turns round: ssdb_heads runs with one SAMPLE per lane, ssdp_unit_add with one HIDDEN UNIT per lane,
// which recomputes its own h_i and u_i from the sample's features (the same fma chains, so the same bits as in ssdb_heads) and adds the sample's terms into the
// SSDP_ACC accumulators of its row.  Every accumulation is a plain fp32 fma or add: the sum of an element is formed in the order in which the samples are handed in.
// Plain C like decode_bwd_math.h: the kernel and the host harness (tests/host/decode_bwd_params_host.c) compile the SAME arithmetic.
#pragma once
#include "decode_bwd_math.h"

#define SSDP_PARAM_FLOATS SSDNERF_MLP_PARAM_FLOATS
// accumulators of hidden unit i, in the order of its record: [0, 18) dW1_i, 18 db1_i, 19 dws_i, 20 .. 22 dWc_{0..2},i; then [23, 39) dWd_i, 39 dbd_i; then the four
// sums that do not depend on i (every unit forms them, identically; unit 0's are stored): 40 dbs, 41 .. 43 dbc
#define SSDP_ACC 44
#define SSDP_ACC_WD 23
#define SSDP_ACC_BD 39
#define SSDP_ACC_TAIL 40

// one sample's terms of hidden unit i, added to the unit's accumulators.  rec = the unit's record (W1_i[18], b1_i, w_s,i, Wc_{0..2},i), wd = Wd_i[16], bd = bd_i
SSDB_FN void ssdp_unit_add(const float rec[23], const float wd[16], float bd, const float f[18], const float sh[16], float dsa, const float dz[3],
                           float acc[SSDP_ACC]) {
    float h = rec[18];
    SSDB_UNROLL
    for (int k = 0; k < 18; ++k) h = fmaf(rec[k], f[k], h);
    float d = bd;
    SSDB_UNROLL
    for (int m = 0; m < 16; ++m) d = fmaf(wd[m], sh[m], d);
    const float sg = ssdb_sigmoid(h);
    const float a = dsa * rec[19] * (sg * fmaf(h, 1.0f - sg, 1.0f));
    const float u = h + d, su = ssdb_sigmoid(u);
    const float dc = fmaf(dz[2], rec[22], fmaf(dz[1], rec[21], dz[0] * rec[20]));
    const float du = su * fmaf(u, 1.0f - su, 1.0f);
    const float e = dc * du;
    const float ae = fmaf(dc, du, a);                                        // a_i + e_i, one rounding: ssdb_mlp_backward's dh_i
    const float s = h * sg, c = u * su;
    SSDB_UNROLL
    for (int k = 0; k < 18; ++k) acc[k] = fmaf(ae, f[k], acc[k]);
    acc[18] += ae;
    acc[19] = fmaf(dsa, s, acc[19]);
    acc[20] = fmaf(dz[0], c, acc[20]);
    acc[21] = fmaf(dz[1], c, acc[21]);
    acc[22] = fmaf(dz[2], c, acc[22]);
    SSDB_UNROLL
    for (int m = 0; m < 16; ++m) acc[SSDP_ACC_WD + m] = fmaf(e, sh[m], acc[SSDP_ACC_WD + m]);
    acc[SSDP_ACC_BD] += e;
    acc[SSDP_ACC_TAIL] += dsa;
    acc[SSDP_ACC_TAIL + 1] += dz[0];
    acc[SSDP_ACC_TAIL + 2] += dz[1];
    acc[SSDP_ACC_TAIL + 3] += dz[2];
}

// the accumulators of hidden unit i -> the packed parameter layout of decode_core.h (Wc transposed into the records; the unused column rec[23] = 0)
SSDB_FN void ssdp_store_row(const float acc[SSDP_ACC], int i, float* __restrict__ grad) {
    SSDB_UNROLL
    for (int k = 0; k < 23; ++k) grad[i * 24 + k] = acc[k];
    grad[i * 24 + 23] = 0.0f;
    SSDB_UNROLL
    for (int m = 0; m < 16; ++m) grad[SSDB_OFF_WD + i * 16 + m] = acc[SSDP_ACC_WD + m];
    grad[SSDB_OFF_BD + i] = acc[SSDP_ACC_BD];
    if (i == 0) {
        SSDB_UNROLL
        for (int q = 0; q < 4; ++q) grad[SSDB_OFF_TAIL + q] = acc[SSDP_ACC_TAIL + q];
    }
}
