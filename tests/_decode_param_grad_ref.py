"""float64 reference of the decode gradient w.r.t. the DECODER's parameters -- ``ssdnerf_point_decode_backward_params`` (csrc/decode_bwd_params.hip:
``k_decode_bwd_params``, ``k_decode_bwd_params_sum``; the arithmetic of csrc/decode_bwd_params_math.h) -- with error bounds derived from the kernel's arithmetic, on the
seeded per-sample families of tests/_decode_grad_ref.py.  Built on ``_decode_grad_ref.decode_grad_terms``: it yields dsa, dz, dh = a + e and the forward's intermediates,
each with its carried bound, in that module's house style (u = 2^-24, first-order forward analysis, second-order remainders added explicitly, each derivation next to its
term, no constant fitted to a GPU run).

Notation of csrc/decode_bwd_params_math.h.  One sample contributes to every parameter element ONE term, a product x y of two per-sample quantities (or x alone, for a
bias), and the element is the sum of its terms over the samples with an upstream gradient:

    dW1_ik = sum (a_i + e_i) f_k     db1_i = sum (a_i + e_i)     dWd_im = sum e_i SH_m     dbd_i = sum e_i
    dws_i  = sum dsa silu(h_i)       dbs   = sum dsa             dWc_ji = sum dz_j silu(u_i)   dbc_j = sum dz_j

Bound of an element:   sum_n (carried bound of the term)  +  (N_live + C_TERM) u sum_n |term|
  * carried bound of a term x y whose factors the kernel holds to within Bx, By:  |y| Bx + |x| By + Bx By  (the two first-order parts and their product; for a bias, Bx);
  * the kernel never rounds a term on its own: acc = fma(x, y, acc) rounds the running sum once per sample.  The first fma (onto 0) is the rounded product, every later
    one a rounded addition: N_live roundings for N_live samples, each at most u times a partial sum, which is at most sum |term| to first order.  This covers ANY
    grouping of the additions -- the lanes' accumulators, the block's four waves, the per-block records and their final sum: n non-zero contributions are joined by
    n - 1 rounded additions however they are grouped, and adding the exact zeros of an idle wave or block rounds nothing;
  * C_TERM = 2: one for the rounded first product, one for the second order of the chain: (1 + u)^N - 1 <= N u (1 + N u / 2 + ...) and N u (N u / 2) sum |term| <=
    u sum |term| while N^2 u <= 2, i.e. N <= 5792; ``MAX_LIVE`` = 4096 is asserted.
An element no sample reaches has bound 0 and must be exactly 0; so must the unused column rec[:, 23] of the packed layout.

Nothing here needs a GPU."""
import functools
from types import SimpleNamespace

import numpy as np

import _decode_grad_ref as G
import _render_ref as RR
from _render_ref import U32

C_TERM = 2.0
MAX_LIVE = 4096
N_PARAMS = 64 * 24 + 64 * 16 + 64 + 4
NAMES = ("base_net.0.weight", "base_net.0.bias", "density_net.0.weight", "density_net.0.bias", "dir_net.0.weight", "dir_net.0.bias", "color_net.0.weight",
         "color_net.0.bias")
MUTATIONS = ("db1-without-e", "dWc-untransposed")


def _sum_of_products(x, Bx, y, By):
    """(value, carried bound, sum |term|) [I, K] of sum_n x[n, i] y[n, k] for factors held to within Bx, By"""
    ax, ay = np.abs(x), np.abs(y)
    return x.T @ y, Bx.T @ ay + ax.T @ By + Bx.T @ By, ax.T @ ay


def _sum(x, Bx):
    return x.sum(0), Bx.sum(0), np.abs(x).sum(0)


def pack(dW1, db1, dws, dbs, dWd, dbd, dWc, dbc, untransposed=False):
    """the eight gradients in the packed parameter layout of csrc/decode_core.h; ``untransposed``: the second control's mistake, dWc [3, 64] copied in its own memory
    order into the [64, 3] slot of the records"""
    rec = np.zeros((64, 24))
    rec[:, :18], rec[:, 18], rec[:, 19] = dW1, db1, np.reshape(dws, 64)
    rec[:, 20:23] = np.reshape(dWc, (64, 3)) if untransposed else np.asarray(dWc).T
    return np.concatenate([rec.reshape(-1), np.reshape(dWd, -1), np.reshape(dbd, -1), np.reshape(dbs, -1), np.reshape(dbc, -1)])


def unpack(g):
    """packed gradient [N_PARAMS] -> {state-dict key: array in the parameter's own shape}"""
    g = np.asarray(g)
    rec = g[:1536].reshape(64, 24)
    return {"base_net.0.weight": rec[:, :18], "base_net.0.bias": rec[:, 18], "density_net.0.weight": rec[:, 19][None], "density_net.0.bias": g[2624:2625],
            "dir_net.0.weight": g[1536:2560].reshape(64, 16), "dir_net.0.bias": g[2560:2624], "color_net.0.weight": rec[:, 20:23].T, "color_net.0.bias": g[2625:2628]}


L3 = 0.5    # |silu'''| = |3 s'' + u s'''| with s = sigmoid: |s''| = |s (1 - s) (1 - 2 s)| <= 0.0963 and |u s'''| = |u s (1 - s) (1 - 6 s + 6 s^2)| <= 0.11: below 0.40
            # everywhere (the CPU module evaluates it on a grid)


def silu3(u):
    """silu'''(u), for the check of ``L3``"""
    s = RR._sig(u)
    s1 = s * (1.0 - s)
    return 3.0 * s1 * (1.0 - 2.0 * s) + u * s1 * (1.0 - 6.0 * s + 6.0 * s * s)


def dsilu_local(h, Bh):
    """``G.dsilu_terms`` with its carried part taken LOCALLY.  That function moves silu' by the global Lipschitz constant max |silu''| = 1/2 (attained at 0) times
    Bh.  A hidden unit whose pre-activation sits far out -- the decoder's shape pathway, unit 0 with b1 = -8 -- has |silu'| ~ 1e-3 there and |silu''| of the same size:
    the global constant overstates its carried error a hundredfold, and every gradient element of that unit's row with it.  By the mean value theorem
        |silu'(h + d) - silu'(h)| <= max over [h - Bh, h + Bh] of |silu''| * |d| <= (|silu''(h)| + L3 Bh) Bh,      silu''(h) = s (1 - s) (2 + h (1 - 2 s)),
    never more than the global form (the smaller of the two is taken).  The kernel's own roundings are ``G.dsilu_terms``', unchanged."""
    D, B = G.dsilu_terms(h, Bh)
    s = RR._sig(h)
    local = (np.abs(s * (1.0 - s) * (2.0 + h * (1.0 - 2.0 * s))) + L3 * Bh) * Bh
    return D, B - 0.5 * Bh + np.minimum(0.5 * Bh, local)


def scene_terms(P, code, xyz, dirs, sat, g_sigma, g_rgb, mutate=None):
    """(value, carried bound, sum |term|), each packed [N_PARAMS], of the samples of ONE scene (all of them with an upstream gradient)"""
    t = G.decode_grad_terms(P, code, xyz, dirs, sat, g_sigma, g_rgb)
    fw, p = t.fwd, t.fwd.p
    dsa, Bdsa = t.dsa[:, None], t.B_dsa[:, None]
    # a_i = fl(fl(dsa w_i) silu'(h_i)): two roundings; the carried errors of both factors and their product (as ``decode_grad_terms``, on ``dsilu_local``)
    D, BD = dsilu_local(fw.h, fw.B_h)
    a = dsa * p.ws * D
    Ba = np.abs(p.ws * D) * Bdsa + np.abs(dsa * p.ws) * BD + np.abs(p.ws) * Bdsa * BD + 2.0 * U32 * np.abs(a)
    # e_i = fl(dc_i silu'(u_i)), dc = dz0 w0, then fma(dz1, w1, .), then fma(dz2, w2, .): the carried errors of both factors, their product, one rounding of the product
    dc = t.dz @ p.Wc
    Bdc = t.B_dz @ np.abs(p.Wc) + G.chain_rounding(t.dz[:, None, :] * p.Wc.T[None], np.zeros((1, 1)))
    Du, BDu = dsilu_local(fw.hc, fw.B_hc)
    e = dc * Du
    Be = np.abs(Du) * Bdc + np.abs(dc) * BDu + Bdc * BDu + U32 * np.abs(e)
    # a_i + e_i = fma(dc_i, silu'(u_i), a_i), one rounding: ``ssdb_mlp_backward``'s dh_i (the value is ``decode_grad_terms``' own)
    ae = t.dh
    assert np.allclose(ae, dc * Du + a, rtol=1e-12, atol=0.0)
    Bae = np.abs(Du) * Bdc + np.abs(dc) * BDu + Bdc * BDu + Ba + U32 * np.abs(ae)
    assert (Bae <= t.B_dh * (1.0 + 1e-12)).all()                             # (never looser than the bound carried there)
    # silu(h_i) = fl(h_i sigmoid(h_i)) and silu(u_i) as the forward forms them: ``RR.silu_terms``
    s, Bs = RR.silu_terms(fw.h, fw.B_h)
    c, Bc = RR.silu_terms(fw.hc, fw.B_hc)
    db1 = _sum(ae - e, Bae) if mutate == "db1-without-e" else _sum(ae, Bae)
    parts = (_sum_of_products(ae, Bae, fw.f, fw.B_f), db1, _sum_of_products(s, Bs, dsa, Bdsa), _sum(dsa, Bdsa), _sum_of_products(e, Be, fw.sh, fw.B_sh), _sum(e, Be),
             _sum_of_products(t.dz, t.B_dz, c, Bc), _sum(t.dz, t.B_dz))
    return tuple(pack(*[q[j] for q in parts], untransposed=(mutate == "dWc-untransposed" and j == 0)) for j in range(3))


def case_reference(c, mutate=None):
    """namespace(ref, bound, mag [N_PARAMS], n_live) of a whole case (``G.sample_case``): the float64 sum over every scene's samples with a gradient"""
    live = (c.g_sigma != 0) | (c.g_rgb != 0).any(1)
    val, carried, mag = np.zeros(N_PARAMS), np.zeros(N_PARAMS), np.zeros(N_PARAMS)
    for s in range(c.S):
        idx = np.arange(int(c.offsets[s]), int(c.offsets[s + 1]))
        idx = idx[live[idx]]
        if len(idx):
            v, b, m = scene_terms(c.P, c.code[s], c.xyz[idx], c.dirs[idx], c.sat, c.g_sigma[idx], c.g_rgb[idx], mutate)
            val, carried, mag = val + v, carried + b, mag + m
    n_live = int(live.sum())
    assert n_live <= MAX_LIVE, ("C_TERM's second-order allowance is derived for at most MAX_LIVE samples", n_live)
    return SimpleNamespace(ref=val, bound=carried + (n_live + C_TERM) * U32 * mag, mag=mag, n_live=n_live)


@functools.lru_cache(maxsize=None)
def reference(name, mutate=None):
    """``case_reference`` of a family of ``G.SAMPLE_FAMILIES``; shared, read-only"""
    return case_reference(G.sample_case(name), mutate)


def check_le(got, ref, bound):
    return G.check_le(got, ref, bound)
