"""Float64 reference of the bias-free ReLU MLP (oracle.tcnn_ref's flat parameter layout) and an error model DERIVED from the
operand formats csrc/mlp_split.hpp and csrc/mlp_half.hpp state -- no measured tolerance, no tuned constant.

Formats (mlp_split.hpp header, split_rows.hpp):
  f16x2   v as hi = f16(v 2^k), lo = f16(v 2^k - hi); k = scale_exp(max |group|) puts the group's maximum in [2^13, 2^14) and is
          clamped to +-110.  hi is within 2^-11 of v 2^k, lo within 2^-11 of the rest: 2^-22 |v|, or -- where lo is an f16
          subnormal -- half its step, 2^-25, in the scaled domain: 2^-25 2^-k.
  f16     the hi part alone (DNS_MLP_FP16, half rows): max(2^-11 |v|, 2^-25 2^-k).
  bf16x3  three bf16 parts, no scale (the weight-gradient products): 2^-23 |v|.
  bf16x2  two bf16 parts (the weight-gradient products of DNS_MLP_FP16): 2^-16 |v|.
A product drops the lo x lo term (2^-22 |a||b|; bf16x3: 2^-23, bf16x2 the m x m term 2^-16) and accumulates in fp32, one rounding
per 16-wide K-step and one for the result: (K / 16 + 1) 2^-24 |a||b|.  The error coming into a layer passes through |W|; ReLU is
1-Lipschitz.

Terms beyond the bare format, each from the kernels' code: a result stored as fp32 may be an fp32 subnormal (+ 2^-149); the
accumulation and dropped-product terms are taken on the COMPUTED operands (|a| + da)(|b| + db), which also carries the second-order
term da db; DNS_MLP_FP16 forms its weight gradients from two bf16 parts and three products (mma_pt, PREC 1), hence "bf16x2";
two input segments with their own exponents are aligned by max(e - e_k, -24) (xs_align), see input_error.

ReLU masks: a hidden unit whose pre-activation lies inside its own bound of zero is UNDETERMINED -- the kernel may pass its
gradient or not.  Its gradient entry is then anywhere between 0 and the full value, so |value| is added to that entry's error and
travels on through |W| into dx and the weight gradients (the term |g_j| |W[j, :]| per such unit).  Where the issue's procedure
applies (near_kink points get dy = 0 on both sides, at most 2 % of the points) the term vanishes with g.

Groups: a weight matrix is one group (its n_out live rows for W_out), activations and gradients one group per POINT.  The
maximum the kernel sees is the maximum of COMPUTED values, so for derived quantities the exponent is taken from the reference
maximum plus its own error bound (an upper bound on the maximum gives a lower bound on k and an upper bound on the subnormal step).
"""
import math

import torch

from oracle import tcnn_ref as tr

D = torch.float64
U24 = 2.0 ** -24
FP32_SUB = 2.0 ** -149

# mode -> (operand format, dropped product term, weight-gradient operand format, its dropped term)
MODES = {
    "exact": ("f16x2", 2.0 ** -22, "bf16x3", 2.0 ** -23),
    "fp16": ("f16", 0.0, "bf16x2", 2.0 ** -16),
    "half": ("f16", 0.0, None, 0.0),          # half rows: no scale (k = 0; gradients k = log2(loss scale)), wgrad on the f16 operands
}


def scale_exp(m: torch.Tensor) -> torch.Tensor:
    """csrc/split_rows.hpp scale_exp on the fp32 value of m: k with m 2^k in [2^13, 2^14), clamped to +-110; 0 for m = 0 or a
    non-finite m.  Returned as float64."""
    m32 = m.to(torch.float32)
    _, ex = torch.frexp(m32)
    k = (14 - ex).clamp(-110, 110)
    ok = (m32 > 0) & torch.isfinite(m32)
    return torch.where(ok, k, torch.zeros_like(k)).to(D)


def operand_error(v, group_max, fmt, slack=0.0, k=None):
    """Absolute representation error the stated format allows for v (float64), element-wise.  group_max broadcasts against v;
    ``slack``: bound on the error of group_max itself; ``k``: a fixed exponent instead of scale_exp(group_max)."""
    a = v.abs().to(D)
    if fmt == "bf16x3":
        return a * 2.0 ** -23
    if fmt == "bf16x2":
        return a * 2.0 ** -16
    if k is None:
        k = scale_exp(torch.as_tensor(group_max, dtype=D) + slack)
    else:
        k = torch.as_tensor(float(k), dtype=D)
    floor = 2.0 ** -25 * torch.exp2(-k)
    rel = {"f16x2": 2.0 ** -22, "f16": 2.0 ** -11}[fmt]
    return torch.maximum(a * rel, floor.expand_as(a))


def mats64(params, shape):
    """[W_in [nn, n_in], W_h ..., W_out [n_out, nn]] in float64 (the padded rows of W_out are storage only)."""
    n_in, n_out, nn, nl = shape
    m = tr.mlp_split(params.detach().to(D).reshape(-1), n_in, n_out, nn, nl)
    return list(m[:-1]) + [m[-1][:n_out]]


def used_count(shape):
    n_in, n_out, nn, nl = shape
    return nn * n_in + (nl - 1) * nn * nn + n_out * nn


def flat_used(mats):
    return torch.cat([m.reshape(-1) for m in mats])


def _prod(absA, dA, absB, dB, drop):
    """Bound on the error of A @ B computed from operands within dA, dB of A, B (K = the contraction width)."""
    K = absA.shape[1]
    hatA, hatB = absA + dA, absB + dB
    return absA @ dB + dA @ hatB + (drop + (math.ceil(K / 16) + 1) * U24) * (hatA @ hatB)


def _rowmax(t):
    return t.abs().amax(dim=1, keepdim=True)


def input_error(X, mode, n1=None, own_exps=False):
    """Bound on the error of the first layer's input operand.  n1 / own_exps: two segments that carry their own exponents
    (split rows), aligned to the smaller one inside the kernel."""
    fmt = MODES[mode][0]
    if mode == "half":
        return torch.zeros_like(X)                          # the rows ARE f16
    if not own_exps:
        return operand_error(X, _rowmax(X), fmt)
    parts = 2.0 if fmt == "f16x2" else 1.0
    e = scale_exp(_rowmax(X))                               # the smaller exponent: that of the larger segment
    align = parts * 2.0 ** -25 * torch.exp2(-e)             # either part may round when it is multiplied down to it
    das = []
    for sgm in (X[:, :n1], X[:, n1:]):
        # xs_align multiplies by 2^max(e - e_k, -24): a segment more than 24 binades below the other is carried
        # 2^(e_k - e - 24) times too large -- at most 2^14 2^-24 in the scaled domain, 2^-23 of the row's maximum
        d = scale_exp(_rowmax(sgm)) - e
        over = torch.where(d > 24, torch.exp2(d - 24) - 1.0, torch.zeros_like(d))
        das.append(operand_error(sgm, _rowmax(sgm), fmt) + over * sgm.abs())
    return torch.cat(das, 1) + align


def emulate_aligned(x1, x2, clamp=-24):
    """the value xs_align leaves in the operand of a two-segment split-row input (exact mode): each segment's hi / lo under its
    own exponent, both multiplied in f16 by 2^max(e - e_k, clamp), e the smaller exponent"""
    segs = [t.detach().to(D) for t in (x1, x2)]
    es = [scale_exp(_rowmax(t)) for t in segs]
    e = torch.minimum(*es)
    out = []
    for t, ek in zip(segs, es):
        sc = t * torch.exp2(ek)
        hi = _q16(sc)
        lo = _q16(sc - hi)
        m = _q16(torch.exp2(torch.clamp(e - ek, min=clamp)))
        out.append((_q16(hi * m) + _q16(lo * m)) * torch.exp2(-e))
    return torch.cat(out, 1)


def _net(X, Ws, dY, mode, n1=None, own_exps=False, loss_scale=128.0):
    """One weight set: reference values and bounds.  X [P, n_in], dY [P, n_out] or None.  n1 / own_exps: see input_error."""
    fmt, drop, wfmt, wdrop = MODES[mode]
    half = mode == "half"
    kf = 0.0 if half else None                              # activations / weights of half rows: plain f16
    kg = math.log2(loss_scale) if half else None            # their gradients: f16 of loss_scale * value
    out = {}
    # ---- forward
    da = input_error(X, mode, n1, own_exps)
    acts, e_acts, d_acts, pres, e_pres, dWq = [X], [torch.zeros_like(X)], [da], [], [], []
    for li, W in enumerate(Ws):
        dWq.append(operand_error(W, W.abs().max(), fmt, k=kf))
        pre = acts[-1] @ W.T
        e_pre = _prod(acts[-1].abs(), d_acts[-1], W.abs().T, dWq[-1].T, drop)
        if li == len(Ws) - 1:
            out["y"], out["e_y"] = pre, e_pre + FP32_SUB
            break
        h = torch.relu(pre)
        pres.append(pre)
        e_pres.append(e_pre)
        acts.append(h)
        e_acts.append(e_pre)
        d_acts.append(e_pre + operand_error(h.abs() + e_pre, _rowmax(h), fmt, slack=e_pre.amax(dim=1, keepdim=True), k=kf))
    out["pre"], out["e_pre"] = pres, e_pres
    if dY is None:
        return out
    # ---- backward
    g, e_g = dY, torch.zeros_like(dY)                       # the fp32 gradient of the layer's output and its error
    d_g = operand_error(dY, _rowmax(dY), fmt, k=kg)         # ... as the operand of the data-gradient product
    dWs, e_dWs = [None] * len(Ws), [None] * len(Ws)
    for li in range(len(Ws) - 1, -1, -1):
        W = Ws[li]
        if half:
            gw, aw = d_g, d_acts[li]                        # the f16 operands that exist anyway
        else:
            gw = e_g + operand_error(g.abs() + e_g, None, wfmt)
            aw = e_acts[li] + operand_error(acts[li].abs() + e_acts[li], None, wfmt)
        dWs[li] = g.T @ acts[li]
        e_dWs[li] = _prod(g.abs().T, gw.T, acts[li].abs(), aw, wdrop) + FP32_SUB
        d_in = g @ W
        e_in = _prod(g.abs(), d_g, W.abs(), dWq[li], drop)
        if li == 0:
            out["dx"], out["e_dx"] = d_in, e_in + FP32_SUB
        else:
            on = pres[li - 1] > 0
            # the kernel masks on ITS activation (half rows: on the f16 it keeps): undetermined inside that operand's error
            und = pres[li - 1].abs() <= (d_acts[li] if half else e_pres[li - 1])
            g = torch.where(on, d_in, torch.zeros_like(d_in))
            e_g = torch.where(und, d_in.abs() + e_in, torch.where(on, e_in, torch.zeros_like(e_in)))
            d_g = e_g + operand_error(g.abs() + e_g, _rowmax(g), fmt, slack=e_g.amax(dim=1, keepdim=True), k=kg)
    out["dW"], out["e_dW"] = dWs, e_dWs
    return out


def analyse(x, params, dy, shape, mode="exact", x2=None, group=None, own_exps=False, min_count=2, loss_scale=128.0):
    """Reference and bounds for a launch.  params: flat [count] or a pool [G, count] with ``group`` [P] (negative: no network;
    groups of fewer than min_count points are skipped: zeros).  x2: the second input segment.  Returns a dict of float64
    tensors: y, dx (dx1, dx2 with two segments), dparams ([used] or [G, used]: W_out's live rows only), pre (list per hidden
    layer) and the bound of each under e_<name>."""
    n_in, n_out, nn, nl = shape
    X = x.detach().to(D) if x2 is None else torch.cat((x.detach().to(D), x2.detach().to(D)), 1)
    n1 = None if x2 is None else x.shape[1]
    dY = None if dy is None else dy.detach().to(D)
    P = X.shape[0]
    if group is None:
        r = _net(X, mats64(params, shape), dY, mode, n1, own_exps, loss_scale)
        res = {"y": r["y"], "e_y": r["e_y"], "pre": r["pre"], "e_pre": r["e_pre"]}
        if dY is not None:
            res.update(dx=r["dx"], e_dx=r["e_dx"], dparams=flat_used(r["dW"]), e_dparams=flat_used(r["e_dW"]))
    else:
        G = params.shape[0]
        z = lambda *s: torch.zeros(*s, dtype=D)
        res = {"y": z(P, n_out), "e_y": z(P, n_out), "pre": [z(P, nn) for _ in range(nl)],
               "e_pre": [torch.full((P, nn), float("inf"), dtype=D) for _ in range(nl)]}
        if dY is not None:
            res.update(dx=z(P, n_in), e_dx=z(P, n_in), dparams=z(G, used_count(shape)), e_dparams=z(G, used_count(shape)))
        for gi in range(G):
            idx = (group == gi).nonzero().reshape(-1)
            if idx.numel() < min_count:
                continue
            r = _net(X[idx], mats64(params[gi], shape), None if dY is None else dY[idx], mode, n1, own_exps, loss_scale)
            res["y"][idx], res["e_y"][idx] = r["y"], r["e_y"]
            for l in range(nl):
                res["pre"][l][idx], res["e_pre"][l][idx] = r["pre"][l], r["e_pre"][l]
            if dY is not None:
                res["dx"][idx], res["e_dx"][idx] = r["dx"], r["e_dx"]
                res["dparams"][gi], res["e_dparams"][gi] = flat_used(r["dW"]), flat_used(r["e_dW"])
    if dY is not None and n1 is not None:
        for k in ("dx", "e_dx"):
            res[k + "1"], res[k + "2"] = res[k][:, :n1], res[k][:, n1:]
    return res


def forward64(x, params, shape, x2=None, group=None):
    """(y, [pre-activation of every hidden layer]) in float64."""
    r = analyse(x, params, None, shape, x2=x2, group=group)
    return r["y"], r["pre"]


def backward64(x, params, dy, shape, x2=None, group=None):
    """dict y, pre, dx (dx1, dx2), dparams (used rows only) in float64."""
    r = analyse(x, params, dy, shape, x2=x2, group=group)
    return {k: v for k, v in r.items() if not k.startswith("e_")}


def error_bound(x, params, dy, shape, mode="exact", x2=None, group=None, own_exps=False, loss_scale=128.0):
    """dict y, pre, dx (dx1, dx2), dparams: the element-wise bound on |kernel - float64| the stated formats allow."""
    r = analyse(x, params, dy, shape, mode, x2, group, own_exps, loss_scale=loss_scale)
    return {k[2:]: v for k, v in r.items() if k.startswith("e_")}


def near_kink(pre_activations, bound):
    """[P] bool: points with a hidden pre-activation inside its own error bound of zero (the ReLU mask is undetermined)."""
    flag = None
    for p, e in zip(pre_activations, bound):
        f = ((p.abs() <= e) & torch.isfinite(e)).any(dim=1)
        flag = f if flag is None else flag | f
    return flag


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an error inside a zero bound must be zero."""
    d = (got.detach().to(D).cpu() - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def assert_within(what, got, ref, bound):
    """|got - ref| <= bound element-wise; the margin used goes on record (util.REPORT -> parity_report.json)."""
    import util
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    r = ratio(got, ref, bound)
    scale = float(ref.abs().max())
    e = float((got.detach().to(D).cpu() - ref).abs().max()) / scale if scale > 0 else 0.0
    util.REPORT.append((what, e, r, 1.0))
    print(f"{what}: worst |err| / bound = {r:.4f}")
    assert r <= 1.0, f"{what}: |err| / bound = {r:.3f} > 1 (derived bound, see tests/mlp_ref.py)"
    return r


# ---- torch emulation of the stated format (exact float64 products) ------------------------------------------------------------
def _q16(s):
    return s.to(torch.float16).to(D)


def _represent(v, k, lo=True):
    s = v * torch.exp2(k)
    hi = _q16(s)
    r = hi + _q16(s - hi) if lo else hi
    return r * torch.exp2(-k)


def _tile_max(m, tile):
    if not tile:
        return m
    out = m.clone()
    for s in range(0, m.shape[0], 32):
        out[s:s + 32] = m[s:s + 32].max()
    return out


def emulate(x, params, dy, shape, lo=True, tile_scale=False):
    """What the exact mode's FORMAT computes when every product and sum is exact: operands as f16 hi (+ lo) under a per-matrix /
    per-point power-of-two scale, weight-gradient operands rounded to 24 bits.  lo=False drops the lo plane; tile_scale=True
    shares one scale among the 32 points of a tile.  Returns y, dx, dparams (used rows)."""
    X, dY, Ws = x.detach().to(D), dy.detach().to(D), mats64(params, shape)
    rep = lambda t: _represent(t, scale_exp(_tile_max(_rowmax(t), tile_scale)), lo)
    Wq = [_represent(W, scale_exp(W.abs().max()), lo) for W in Ws]
    f32 = lambda t: t.to(torch.float32).to(D)
    acts = [X]
    for Wk in Wq[:-1]:
        acts.append(torch.relu(rep(acts[-1]) @ Wk.T))
    y = rep(acts[-1]) @ Wq[-1].T
    g, dWs = dY, [None] * len(Ws)
    for li in range(len(Ws) - 1, -1, -1):
        dWs[li] = f32(g).T @ f32(acts[li])
        d_in = rep(g) @ Wq[li]
        if li:
            g = torch.where(acts[li] > 0, d_in, torch.zeros_like(d_in))
    return y, d_in, flat_used(dWs)


# ---- the input sets of the range tests ---------------------------------------------------------------------------------------
NETS = [(80, 33, 64, 2), (112, 8, 32, 1), (16, 64, 32, 2)]
N1 = {80: 16, 112: 48, 16: 8}                              # first segment of the two-segment forms, by n_in
P_POINTS = 101                                             # three full 32-point tiles and a 5-point tail
IN_ROW = [(r, inv) for r in (-12, -20, -30) for inv in (False, True)]
FINITE = ["rows", "clamp", "weights"] + [f"inrow{r}{'w' if inv else ''}" for r, inv in IN_ROW]
# Cases built to reach the f16 subnormal step of the stated format (operand_error's second term).  A weight row 2^-30 below its
# matrix's maximum, or an input column 2^-30 below its row's, is scaled to 2^-17: the step 2^-24 leaves it 2^-8 of ITS OWN
# magnitude.  The outputs stay inside the bound (it is absolute: 2^-38 of the group's maximum), but a hidden unit fed by such
# operands has a pre-activation bound of 1e-3 .. 1e-1 of its typical value, so the share of near-kink points cannot be brought
# under 2 % by the choice of a seed (5-8 of 101 points for "weights", 63-101 for "inrow-30w", any seed); nor can it in the f16
# modes, whose pre-activation bound is 2^-11 of sum |W||x|.  There every point KEEPS its dy and the bound carries the
# undetermined-unit term (module docstring): all 101 points' dx and every weight gradient are held to it.
FORMAT_LIMITED = {"weights", "inrow-30w"}


def base_inputs(shape, seed, P=P_POINTS):
    """unit-scale x, params (padded rows of W_out zero, as the ABI keeps them) and dy"""
    n_in, n_out, nn, nl = shape
    g = torch.Generator().manual_seed(seed)
    params = tr.mlp_init(n_in, n_out, nn, nl, g)
    params[used_count(shape):] = 0.0
    return torch.randn(P, n_in, generator=g), params, torch.randn(P, n_out, generator=g)


def param_mats(params, shape):
    """writable fp32 views of the matrices of a flat parameter vector (W_out with its padded rows)"""
    return tr.mlp_split(params, *shape)


def finite_case(name, shape, seed):
    """x, params, dy (fp32) of a single-segment, single-set finite case."""
    n_in, n_out, nn, nl = shape
    x, params, dy = base_inputs(shape, seed)
    P = x.shape[0]
    g = torch.Generator().manual_seed(seed + 1000)
    if name == "rows":                                      # neighbours in a tile differ by up to 120 binades
        e = torch.linspace(-60, 60, P).round()[torch.randperm(P, generator=g)]
        q = torch.linspace(-60, 60, P).round()[torch.randperm(P, generator=g)]
        x, dy = x * torch.exp2(e)[:, None], dy * torch.exp2(q)[:, None]
    elif name == "clamp":                                   # exponent 14 + 120 = 134 is clamped to 110
        for p in (3, 40):
            x[p] *= 2.0 ** -120 / float(x[p].abs().max())
        for p in (7, 40):
            dy[p] *= 2.0 ** -120 / float(dy[p].abs().max())
    elif name == "weights":                                 # rows of a matrix over 30 binades; matrices 80 binades apart
        mats = param_mats(params, shape)
        for M in mats:
            M *= torch.exp2(-(torch.arange(M.shape[0]) % 31).float())[:, None]
        mats[0] *= 2.0 ** 40
        mats[1] *= 2.0 ** -40
    elif name.startswith("inrow"):                          # a wide range inside one row: the lo part underflows f16
        inv = name.endswith("w")
        r = int(name[5:-1] if inv else name[5:])
        nc = min(32, n_in // 2)
        x[:, n_in - nc:] *= 2.0 ** r
        if inv:                                             # ... and the small operands carry the result
            param_mats(params, shape)[0][:, n_in - nc:] *= 2.0 ** -r
    else:
        raise KeyError(name)
    return x, params, dy


def two_segment_case(shape, n1, seed):
    """segment magnitudes in ratio 2^-10, 2^-20, 2^-30 by row; which segment is the small one alternates"""
    x, params, dy = base_inputs(shape, seed)
    p = torch.arange(x.shape[0])
    r = torch.exp2(torch.tensor([-10.0, -20.0, -30.0])[p % 3])[:, None]
    first = ((p // 3) % 2 == 1)[:, None]
    x1 = torch.where(first, x[:, :n1] * r, x[:, :n1]).contiguous()
    x2 = torch.where(first, x[:, n1:], x[:, n1:] * r).contiguous()
    return x1, x2, params, dy


def group_case(shape, seed, G=4):
    """a pool of 4 sets, set g scaled by 2^(20 g - 30); set 3 has a single point (skipped: zeros), one point has no set"""
    n_in, n_out, nn, nl = shape
    x, _, dy = base_inputs(shape, seed)
    pool = torch.stack([base_inputs(shape, seed + 1 + gi)[1] * 2.0 ** (20 * gi - 30) for gi in range(G)])
    P = x.shape[0]
    slot = torch.randint(0, 3, (P,), generator=torch.Generator().manual_seed(seed + 7))
    slot[11] = 3
    slot[50] = -1
    return x, pool, dy, slot


def mask_kinks(dy, pres, e_pres, zero=True):
    """dy with the rows of near-kink points zeroed (zero=False: kept), and the flags"""
    k = near_kink(pres, e_pres)
    dy = dy.clone()
    if zero:
        dy[k] = 0.0
    return dy, k


def kinks_zeroed(mode, name=None):
    """the issue's procedure (zero dy of near-kink points, share <= 2 %) where the format allows it; else the points keep their dy"""
    return mode == "exact" and name not in FORMAT_LIMITED
