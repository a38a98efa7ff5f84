"""Float64 host reference of the fused mapper / tracker losses (csrc/losses.hip), the named test cases, and the mutants.

TEST INFRASTRUCTURE, no GPU import.  Three things live here:

* ``reference(case, dtype)``: the loss terms from the formulas of ``oracle/render_math.py`` (pinned to the modelled project's
  recorded outputs by tests/test_oracle_golden.py) and their gradients from CPU autograd.  A ray's validity is expressed by
  DROPPING the invalid rays and their points and applying the plain formulas to what is left; gradients are scattered back
  to the full shapes with zeros at the dropped rays.  The three comparisons ``z < d - trunc``, ``z > d + trunc`` and
  ``d > 0`` are evaluated on the fp32 values (as torch and the kernel do); everything else runs in ``dtype``.  Call forms:
  an upstream scalar ``g_total``, the occupancy pass-through ``d_occ`` (added into column 0 of ``d_fine`` for EVERY point,
  valid or not), and (in the GPU test) a destination leading dimension ``ldd_fine >= L``.
  ``dtype=torch.float32`` is the yardstick: the same formulas in fp32 on the CPU.
* ``CASES``: name -> builder of a ``Case`` (seeded ``torch.Generator``, CPU tensors), shared by the GPU test and the CPU
  self-test.  Large values sit in exactly the elements a wrong kernel would skip or misattribute.
* ``mutant(case, name, ref)``: the float64 result a kernel would give if it mishandled one edge.  It is a second,
  independent formulation (per-element masks and weights over the flat arrays, as a kernel walks them); with no mutation
  it must reproduce ``reference`` (tests/test_losses_ref.py checks that), with one it must differ from it by at least
  100x the tolerance the GPU test applies.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import torch

from oracle import render_math as rm

RTOL = 1e-4        # tests/util.py RTOL (BASELINE.json); the cap of every bound
FLOOR = 1e-5       # the bound the existing loss tests hold against fp32 torch
TERMS = ("p", "d", "l", "lt", "fs", "op", "total")
LAMBDAS = (5.0, 5.0, 0.1, 10.0, 10.0, 10.0, 0.2, 0.05)      # p, d, l, lt, fs, op, truncation, sigma
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "get_opacity_loss.npz")

# forward trips of the point kernels (csrc/losses.hip): workgroups x threads x quads per trip, in ELEMENTS
FWD_TRIP = 1024 * 256 * 4 * 4
BWD_TRIP = 4096 * 256 * 2 * 4


class Case:
    """One problem.  Tensors are CPU fp32 (labels int64, valid bool or None = every ray valid)."""

    def __init__(self, name, **kw):
        self.name = name
        self.tracker = False
        self.g_total = 1.0
        self.lam = LAMBDAS
        self.valid = None
        self.d_occ = None          # [P] or None
        self.unaligned = ()        # subset of ("fine", "coarse", "d_coarse"): views 4 bytes into a larger buffer
        self.boundary = False      # the one case that puts z exactly on d +- trunc
        self.edges = {}            # mutant name -> the quantities it must move
        self.__dict__.update(kw)

    @property
    def P(self):
        return self.N * self.S

    @property
    def E(self):
        return self.N * self.S * self.L

    @property
    def quads(self):
        """Elements the PARENT float4 path would cover: aligned fine / coarse -> all but the last E % 4."""
        return 0 if ("fine" in self.unaligned or "coarse" in self.unaligned) else self.E // 4 * 4

    def grad_names(self):
        if self.tracker:
            return ("d_color", "d_depth", "d_var") + (("d_logits",) if self.C else ())
        return ("d_color", "d_depth") + (("d_logits",) if self.C else ()) + ("d_fine", "d_coarse")


# ------------------------------------------------------------------------------------------------------ the reference
def band_masks(z32, d32, trunc):
    """front / back / depth masks of utils/common.py:776-779 on the fp32 values, as bool [n, S], [n, S], [n, 1]."""
    t32 = torch.tensor(float(trunc), dtype=torch.float32)
    d = d32.to(torch.float32).unsqueeze(-1)
    z = z32.to(torch.float32)
    return z < (d - t32), z > (d + t32), d > 0.0


def opacity_terms(z32, d32, occ_logit, trunc, sigma, force_flag=False):
    """oracle/render_math.py opacity_loss with the comparisons on fp32 and the rest in occ_logit.dtype."""
    dt = occ_logit.dtype
    front, back, dm = band_masks(z32, d32, trunc)
    front, back, dm = front.to(dt), back.to(dt), dm.to(dt)
    occ = torch.sigmoid(10 * occ_logit).reshape(z32.shape)
    omask = (1.0 - front) * (1.0 - back) * dm
    zero = torch.zeros((), dtype=dt)
    if force_flag or (torch.count_nonzero(front) > 0 and torch.count_nonzero(omask) > 0):
        fs = ((occ * front * dm) ** 2).mean()
        pseudo = 0.5 * torch.exp(-0.5 * ((z32.to(dt) - d32.to(dt).unsqueeze(-1)) / sigma) ** 2)
        op = ((occ * omask - pseudo * omask) ** 2).mean()
        return fs, op
    return zero, zero


def reference(case: Case, dtype=torch.float64):
    """-> {"terms": {name: 0-d tensor}, "grads": {name: full-shape tensor}} in ``dtype``."""
    c = case
    keep = torch.arange(c.N) if c.valid is None else torch.nonzero(c.valid).reshape(-1)
    nk = keep.numel()

    def leaf(t):
        return t[keep].to(dtype).clone().requires_grad_(True)

    pc, pd = leaf(c.pred_color), leaf(c.pred_depth)
    pv = leaf(c.pred_var) if c.tracker else None
    lg = leaf(c.logits) if c.C else None
    gc, gd32, lab = c.gt_color[keep].to(dtype), c.gt_depth[keep], c.gt_label[keep]
    gd = gd32.to(dtype)
    lam = c.lam
    zero = torch.zeros((), dtype=dtype)
    nan = torch.full((), float("nan"), dtype=dtype)
    fine = coarse = None
    if c.tracker:
        mask = torch.ones(nk, dtype=torch.bool)
        p = rm.track_photometric_loss(gc, pc, mask)
        d = rm.track_depth_loss(gd, pd, pv, mask)
        l = (rm.track_label_loss(lab, lg, mask) if nk else nan) if c.C else zero
        lt = fs = op = zero
    else:
        p = rm.photometric_loss(gc, pc)
        d = rm.depth_loss(gd, pd)
        l = (rm.label_loss(lab, lg) if nk else nan) if c.C else zero            # the mean over no ray is 0/0
        fine = c.fine.reshape(c.N, c.S, c.L)[keep].to(dtype).clone().requires_grad_(True)
        coarse = c.coarse.reshape(c.N, c.S, c.L)[keep].to(dtype).clone().requires_grad_(True)
        lt = rm.latent_loss(coarse, fine)
        fs, op = opacity_terms(c.z[keep], gd32, fine[..., -1], lam[6], lam[7])
    total = lam[0] * p + lam[1] * d + lam[2] * l + lam[3] * lt + lam[4] * fs + lam[5] * op
    if nk and total.requires_grad:
        total.backward(torch.tensor(float(c.g_total), dtype=dtype))

    def scatter(t, shape):
        out = torch.zeros(shape, dtype=dtype)
        if t is not None and t.grad is not None:
            out[keep] = t.grad
        return out

    grads = {"d_color": scatter(pc, (c.N, 3)), "d_depth": scatter(pd, (c.N,))}
    if c.tracker:
        grads["d_var"] = scatter(pv, (c.N,))
    if c.C:
        grads["d_logits"] = scatter(lg, (c.N, c.C))
    if not c.tracker:
        d_fine = scatter(fine, (c.N, c.S, c.L)).reshape(c.P, c.L)
        if c.d_occ is not None:
            d_fine[:, 0] += c.d_occ.to(dtype)
        grads["d_fine"] = d_fine
        grads["d_coarse"] = scatter(coarse, (c.N, c.S, c.L)).reshape(c.P, c.L)
    terms = dict(zip(TERMS, (p, d, l, lt, fs, op, total)))
    return {"terms": {k: v.detach().to(dtype) for k, v in terms.items()}, "grads": grads}


def without_d_occ(case: Case, ref):
    """The reference for a route that has no occupancy pass-through (ops.mapping_losses): d_fine less d_occ in column 0."""
    if case.tracker or case.d_occ is None:
        return ref
    g = dict(ref["grads"])
    g["d_fine"] = g["d_fine"].clone()
    g["d_fine"][:, 0] -= case.d_occ.to(g["d_fine"].dtype)
    return {"terms": ref["terms"], "grads": g}


# --------------------------------------------------------------------------------------- errors, yardstick and bounds
def scalar_err(a, b) -> float:
    """|a - b| / |b| (absolute where b == 0); 0 where both are NaN, inf where only one is."""
    a, b = float(a), float(b)
    if np.isnan(a) or np.isnan(b):
        return 0.0 if (np.isnan(a) and np.isnan(b)) else float("inf")
    return abs(a - b) / abs(b) if b != 0.0 else abs(a - b)


def tensor_err(a, b, groups=None) -> float:
    """The smallest rtol at which tests/util.py assert_close(a, b, rtol, groups=groups) passes: the larger of the
    scale-relative error and the worst |a-b| / (|b| + group RMS)."""
    from util import elem_err, rel_err
    if b.numel() == 0:
        return 0.0
    if not torch.isfinite(b).all():
        return elem_err(a, b, rtol=1.0, groups=groups)
    return max(rel_err(a, b), elem_err(a, b, rtol=1.0, groups=groups))


def grad_groups(name):
    """Per-column scales for the [P, L] gradients (column 0 carries d_occ, the last column the occupancy terms)."""
    return 1 if name in ("d_fine", "d_coarse") else None


def bound_from(err: float) -> float:
    """max(1e-5, 4 x the fp32-CPU-vs-float64 error), never above RTOL.  1e-5 is what the existing loss tests hold against
    fp32 torch; the factor 4 allows for another summation order."""
    return min(RTOL, max(FLOOR, 4.0 * err))


def yardstick(case: Case, ref=None):
    """Error of the fp32 CPU evaluation of the same formulas against float64, per term and per gradient tensor."""
    ref = ref if ref is not None else reference(case)
    r32 = reference(case, torch.float32)
    err = {t: scalar_err(r32["terms"][t], ref["terms"][t]) for t in TERMS}
    for g in case.grad_names():
        err[g] = tensor_err(r32["grads"][g], ref["grads"][g], grad_groups(g))
    return err


def bounds(case: Case, ref=None):
    return {k: bound_from(v) for k, v in yardstick(case, ref).items()}


# ------------------------------------------------------------------------------------------------------------ mutants
MUTANTS = ("tail_dropped", "quad_first_point", "straddle_validity", "flag_forced", "depth_mask_ignored", "d_occ_valid_only",
           "second_trip_dropped")


def masked_terms(case: Case, mutation=None):
    """The seven terms in float64 from per-element weights over the flat arrays (sums of numerators and counts, then the
    masked means), optionally with one edge mishandled.  Nothing is dropped here: invalid rays get weight 0."""
    c = case
    f64 = torch.float64
    valid = torch.ones(c.N, dtype=torch.bool) if c.valid is None else c.valid.bool()
    vd = valid.to(f64)
    nv = vd.sum()
    gd, pd = c.gt_depth.to(f64), c.pred_depth.to(f64)
    sp = (vd[:, None] * (c.gt_color.to(f64) - c.pred_color.to(f64)) ** 2).sum()
    if c.tracker:
        sd, nd = (vd * (gd - pd).abs() / torch.sqrt(c.pred_var.to(f64) + 1e-10)).sum(), nv
    else:
        dmr = torch.ones(c.N, dtype=f64) if mutation == "depth_mask_ignored" else (c.gt_depth > 0).to(f64)
        sd, nd = (vd * dmr * (gd - pd).abs()).sum(), (vd * dmr).sum()
    p, d = sp / (3.0 * nv), sd / nd
    if c.C:
        lg = c.logits.to(f64)
        l = (vd * (torch.logsumexp(lg, 1) - lg.gather(1, c.gt_label[:, None])[:, 0])).sum() / nv
    else:
        l = torch.zeros((), dtype=f64)
    lt = fs = op = torch.zeros((), dtype=f64)
    if not c.tracker:
        E, L, S = c.E, c.L, c.S
        e = torch.arange(E)
        ray = (e // L) // S
        v = valid[ray]
        in_quad = e < c.quads
        if mutation == "straddle_validity":                    # every element of a quad takes its FIRST element's ray
            ray0 = ((e // 4 * 4) // L) // S
            v = torch.where(in_quad, valid[ray0], v)
        w = v.to(f64)
        if mutation == "tail_dropped":
            w = w * (e < E // 4 * 4).to(f64)
        if mutation == "second_trip_dropped":
            w = w * (~(in_quad & (e >= FWD_TRIP))).to(f64)
        f, co = c.fine.reshape(-1).to(f64), c.coarse.reshape(-1).to(f64)
        slt = (w * (co - f) ** 2).sum()
        e_last = torch.arange(c.P) * L + (L - 1)               # each point's last channel
        wl = w[e_last]
        if mutation == "quad_first_point":                     # of the points that end in a quad, only the quad's first point
            q0 = e_last // 4 * 4
            wl = wl * ((e_last >= c.quads) | (torch.arange(c.P) == q0 // L)).to(f64)
        front, back, dm = band_masks(c.z, c.gt_depth, c.lam[6])
        front, back = front.reshape(-1).to(f64), back.reshape(-1).to(f64)
        dm = dm.expand(c.N, S).reshape(-1).to(f64)
        om = (1.0 - front) * (1.0 - back) * dm
        occ = torch.sigmoid(10.0 * f[e_last])
        zz, dd = c.z.reshape(-1).to(f64), c.gt_depth.to(f64)[:, None].expand(c.N, S).reshape(-1)
        pseudo = 0.5 * torch.exp(-0.5 * ((zz - dd) / c.lam[7]) ** 2)
        sfs = (wl * (occ * front * dm) ** 2).sum()
        sop = (wl * (occ * om - pseudo * om) ** 2).sum()
        flag = ((wl * front).sum() > 0 and (wl * om).sum() > 0) or mutation == "flag_forced"
        npts = nv * S
        lt = slt / (npts * L)
        if flag:
            fs, op = sfs / npts, sop / npts
    lam = c.lam
    total = lam[0] * p + lam[1] * d + lam[2] * l + lam[3] * lt + lam[4] * fs + lam[5] * op
    return dict(zip(TERMS, (p, d, l, lt, fs, op, total)))


def mutant(case: Case, name: str, ref):
    """quantity -> the float64 value a kernel mishandling edge ``name`` would return (terms, and the gradient tensors the
    edge moves directly)."""
    out = dict(masked_terms(case, name))
    c = case
    if name == "d_occ_valid_only" and c.d_occ is not None:
        valid = torch.ones(c.N, dtype=torch.bool) if c.valid is None else c.valid.bool()
        pv = valid[:, None].expand(c.N, c.S).reshape(-1)
        g = ref["grads"]["d_fine"].clone()
        g[:, 0] -= torch.where(pv, torch.zeros(c.P, dtype=g.dtype), c.d_occ.to(g.dtype))
        out["d_fine"] = g
    if name == "tail_dropped" and not c.tracker:
        g = ref["grads"]["d_coarse"].clone().reshape(-1)
        g[c.E // 4 * 4:] = 0.0
        out["d_coarse"] = g.reshape(c.P, c.L)
    return out


def separation(case: Case, name: str, ref, bnd):
    """quantity -> (distance of the mutant from the reference) / (the bound the GPU test applies to that quantity)."""
    from util import rel_err
    m = mutant(case, name, ref)
    out = {}
    for q in case.edges[name]:
        if q in TERMS:
            out[q] = scalar_err(m[q], ref["terms"][q]) / bnd[q]
        else:
            out[q] = rel_err(m[q], ref["grads"][q]) / bnd[q]
    return out


# -------------------------------------------------------------------------------------------------------------- cases
def _alternate(N):
    """valid, invalid, ... counted from the END, so that the last ray (the tail's) is always valid."""
    return (torch.arange(N - 1, -1, -1) % 2) == 0


def make_case(name, N, S, L, C=8, tracker=False, seed=0, valid="alternate", zero_depth="some", d_occ=True, lam=LAMBDAS,
              g_total=1.0, unaligned=(), pred_var=None):
    """The generic problem.  Every z is at least 0.05 away from d +- trunc; sample s of ray n is in front of / inside /
    behind the band by (n // 2 + s) % 3, so that small shapes still have front AND in-band samples on valid rays."""
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    rn = lambda *s: torch.randn(*s, generator=g)
    v = {"alternate": _alternate(N), "all": None, "none": torch.zeros(N, dtype=torch.bool),
         "random": None}[valid] if isinstance(valid, str) else valid
    if isinstance(valid, str) and valid == "random":
        v = r(N) > 0.2
        v[-1] = True
    gd = r(N) * 1.7 + 0.8
    n = torch.arange(N)
    if zero_depth == "some":
        gd[(n % 6 == 1) | (n % 6 == 4)] = 0.0               # one invalid and one valid ray of every six (alternating validity)
    elif zero_depth == "all":
        gd[:] = 0.0
    pd = gd + rn(N) * 0.1
    pd[gd == 0] = 5.0                                        # large where a kernel ignoring d > 0 would count it
    c = Case(name, N=N, S=S, L=L, C=C, tracker=tracker, lam=tuple(lam), g_total=g_total, valid=v, unaligned=tuple(unaligned),
             pred_color=r(N, 3), gt_color=r(N, 3), gt_depth=gd, pred_depth=pd,
             logits=rn(N, max(C, 1))[:, :C].contiguous(), gt_label=torch.randint(0, max(C, 1), (N,), generator=g))
    if tracker:
        c.pred_var = r(N) + 0.01 if pred_var is None else torch.full((N,), float(pred_var))
        c.pred_depth = gd + rn(N) * 0.1
        c.S, c.L = 1, 1
        c.fine = c.coarse = c.z = None
        return c
    kind = (n[:, None] // 2 + torch.arange(S)[None, :]) % 3
    vv = torch.ones(N, dtype=torch.bool) if v is None else v
    if L < 4:
        # narrow latents: the points that END in an aligned quad without being its first point are, in turn, in front of
        # and inside the band -- what a kernel that lets only the quad's first point contribute would lose of fs AND op
        pt = torch.arange(N * S)
        later = (pt != ((pt * L + L - 1) // 4 * 4) // L) & (vv & (gd > 0))[pt // S]
        kf = kind.reshape(-1)
        kf[later] = torch.arange(int(later.sum())) % 2
        kind = kf.reshape(N, S)
    u = r(N, S)
    off = torch.where(kind == 0, -0.3 - 0.2 * u, torch.where(kind == 1, 0.3 * u - 0.15, 0.3 + 0.5 * u))
    z = gd[:, None] + off
    z[gd == 0] = (0.5 + u)[gd == 0]
    c.z = z.contiguous()
    P, E = N * S, N * S * L
    fine = rn(P, L) * 0.3
    diff = rn(P, L)
    flat = diff.reshape(-1)
    ray_of = (torch.arange(E) // L) // S
    first3 = (torch.arange(E) - ray_of * S * L) < 3
    flat[first3] = 10.0                                      # the elements a quad straddling INTO this ray would misattribute
    flat[~vv[ray_of]] = 30.0                                 # invalid rays: must not be seen at all
    if E % 4:
        flat[E // 4 * 4:] = max(3.0, float(np.sqrt(E / (E % 4))))          # the tail weighs about as much as all the rest
    c.fine, c.coarse = fine.contiguous(), (fine + diff).contiguous()
    if d_occ:
        nvalid = max(int(vv.sum()), 1)
        scale = 2.0 * lam[3] / (nvalid * S * L) if lam[3] else 1e-2
        dz = rn(P) * scale
        dz[~vv[torch.arange(P) // S]] *= 3.0                 # the part a kernel adding d_occ at valid rays only would lose
        c.d_occ = dz
    _declare_edges(c)
    return c


def _declare_edges(c: Case):
    """Which mutants this case must tell from the truth, and through which quantities."""
    if c.tracker:
        return
    vv = torch.ones(c.N, dtype=torch.bool) if c.valid is None else c.valid.bool()
    e = {}
    if c.quads and c.E % 4 and bool(vv[-1]):
        e["tail_dropped"] = ["lt", "d_coarse"]
    if c.quads and c.L < 4 and c.E >= 4 and float(reference(c)["terms"]["fs"]) != 0.0:
        e["quad_first_point"] = ["fs", "op"]
    if c.quads and c.valid is not None and (c.S * c.L) % 4 and c.N > 1 and bool(vv.any()) and not bool(vv.all()):
        e["straddle_validity"] = ["lt"]
    if bool((vv & (c.gt_depth == 0)).any()) and bool((vv & (c.gt_depth > 0)).any()):
        e["depth_mask_ignored"] = ["d"]
    if c.d_occ is not None and not bool(vv.all()):
        e["d_occ_valid_only"] = ["d_fine"]
    if c.quads > FWD_TRIP:
        e["second_trip_dropped"] = ["lt", "fs", "op"]
    c.edges = e


def golden_case(ci: int) -> Case:
    """Case ``ci`` of tests/golden/get_opacity_loss.npz (N=11, S=47, L=1; recorded from get_opacity_loss of the modelled
    project with weights 3 and 7 on fs and op): the occupancy logits are the whole latent, the other lambdas are zero."""
    g = np.load(GOLDEN)
    p = f"c{ci}_"
    z, depth, occ = torch.from_numpy(g[p + "z"]), torch.from_numpy(g[p + "depth"]), torch.from_numpy(g[p + "occ"])
    N, S = z.shape
    c = make_case(f"golden_c{ci}", N, S, 1, seed=50 + ci, valid="all", zero_depth="none", d_occ=False,
                  lam=(0.0, 0.0, 0.0, 0.0, 3.0, 7.0, float(g[p + "trunc"]), 0.05))
    c.z, c.gt_depth = z.contiguous(), depth.contiguous()
    c.fine = occ.reshape(N * S, 1).contiguous()
    c.coarse = c.fine.clone()
    c.recorded = {"fs": float(g[p + "fs"]), "op": float(g[p + "op"]),
                  "grad_occ": torch.from_numpy(g[p + "grad_occ"]).reshape(N * S, 1) if p + "grad_occ" in g.files else None}
    _declare_edges(c)
    if ci < 2:
        c.edges = {"quad_first_point": ["fs", "op"]}
    else:
        c.edges = {}
    return c


def _ce(kind):
    C = {"C1": 1, "C0": 0, "C40": 40}.get(kind, 8)
    c = make_case(f"ce_{kind}", 37, 2, 5, C=C, seed=60 + len(kind))
    if kind == "pm80":                                       # log-sum-exp stability: the label sits on the smallest logit
        g = torch.Generator().manual_seed(61)
        c.logits = (torch.rand(37, 8, generator=g) * 160.0 - 80.0).contiguous()
        c.logits[:, 0], c.logits[:, 1] = 80.0, -80.0
        c.gt_label = torch.argmin(c.logits, 1)
    if kind == "equal":
        c.logits = torch.full((37, 8), 3.25)
    return c


def _depth_equal():
    c = make_case("depth_equal", 37, 2, 5, seed=70)
    c.pred_depth[::3] = c.gt_depth[::3]                      # |.|' = 0 there, as torch's abs
    return c


def _trk_var(var):
    c = make_case(f"trk_var_{var:g}", 37, 1, 1, tracker=True, seed=71, valid="random", pred_var=var)
    c.pred_depth[::3] = c.gt_depth[::3]
    return c


def _occ_pm20():
    c = make_case("occ_pm20", 37, 3, 5, seed=72)
    g = torch.Generator().manual_seed(73)
    sign = (torch.rand(c.P, generator=g) > 0.5).float() * 2 - 1
    d = c.coarse - c.fine
    c.fine[:, -1] = 20.0 * sign                              # exp(-10 f) overflows to inf on one side
    c.fine[::5, -1] = torch.randn(c.fine[::5].shape[0], generator=g) * 0.3
    c.coarse = (c.fine + d).contiguous()
    _declare_edges(c)
    return c


def _occ_boundary():
    c = make_case("occ_boundary", 37, 4, 5, seed=74)
    c.boundary = True
    t32 = torch.tensor(c.lam[6], dtype=torch.float32)
    pos = c.gt_depth > 0
    c.z[pos, 0] = (c.gt_depth - t32)[pos]                    # NOT z < d - trunc: in the band
    c.z[pos, 1] = (c.gt_depth + t32)[pos]                    # NOT z > d + trunc: in the band
    _declare_edges(c)
    return c


def _no_front():
    c = make_case("no_front", 12, 3, 5, seed=75)
    front, _, _ = band_masks(c.z, c.gt_depth, c.lam[6])
    c.z = torch.where(front, c.gt_depth[:, None] + 0.05, c.z).contiguous()      # in-band samples only (and behind)
    _declare_edges(c)
    c.edges["flag_forced"] = ["op"]
    return c


def _no_band():
    c = make_case("no_band", 12, 3, 5, seed=76)
    front, back, dm = band_masks(c.z, c.gt_depth, c.lam[6])
    band = ~front & ~back & dm
    c.z = torch.where(band, c.gt_depth[:, None] - 0.35, c.z).contiguous()       # front (and behind) only
    _declare_edges(c)
    c.edges["flag_forced"] = ["fs"]
    return c


def _build_cases():
    cases = {}

    def add(name, fn):
        assert name not in cases, name
        cases[name] = functools.lru_cache(maxsize=None)(fn)

    k = 0
    for L in (1, 2, 3, 4, 5, 7, 33):
        for S in (1, 2, 5):
            k += 1
            add(f"L{L}_S{S}", functools.partial(make_case, f"L{L}_S{S}", 6, S, L, seed=k))
    for ci in range(3):
        add(f"golden_c{ci}", functools.partial(golden_case, ci))
    for N, S, L in ((5, 3, 33), (7, 5, 33), (3, 1, 33), (1, 1, 1), (5, 5, 5), (3, 2, 33)):     # E % 4 = 3, 3, 3, 1, 1, 2
        add(f"tail_{N}_{S}_{L}", functools.partial(make_case, f"tail_{N}_{S}_{L}", N, S, L, seed=30 + N + S))
    for N, S, L in ((9, 4, 33), (5, 3, 33)):
        for which in (("fine",), ("coarse",), ("d_coarse",), ("fine", "coarse", "d_coarse")):
            nm = f"unaligned_{'all' if len(which) == 3 else which[0]}_{N}_{S}_{L}"
            add(nm, functools.partial(make_case, nm, N, S, L, seed=40 + N, unaligned=which))
    for N in (1, 255, 256, 257, 1023, 1024, 1025, 2049):
        add(f"rays_map_{N}", functools.partial(make_case, f"rays_map_{N}", N, 2, 5, seed=80 + N % 7, valid="random"))
        add(f"rays_trk_{N}", functools.partial(make_case, f"rays_trk_{N}", N, 1, 1, tracker=True, seed=90 + N % 7, valid="random"))
    for kind in ("pm80", "equal", "C1", "C0", "C40"):
        add(f"ce_{kind}", functools.partial(_ce, kind))
    add("depth_equal", _depth_equal)
    for var in (0.0, 1e-12, 1e4):
        add(f"trk_var_{var:g}", functools.partial(_trk_var, var))
    add("occ_pm20", _occ_pm20)
    add("occ_boundary", _occ_boundary)
    add("all_depth_zero", functools.partial(make_case, "all_depth_zero", 12, 3, 5, seed=77, zero_depth="all"))
    add("no_front", _no_front)
    add("no_band", _no_band)
    add("all_invalid", functools.partial(make_case, "all_invalid", 12, 3, 5, seed=78, valid="none"))
    add("trk_all_invalid", functools.partial(make_case, "trk_all_invalid", 12, 1, 1, tracker=True, seed=79, valid="none"))
    add("g_0.7", functools.partial(make_case, "g_0.7", 12, 3, 5, seed=81, g_total=0.7))
    add("g_-2", functools.partial(make_case, "g_-2", 12, 3, 5, seed=82, g_total=-2.0))
    return cases


CASES = _build_cases()
# the two second-trip problems (E > one trip of the forward / the point-backward grid-stride loop, E % 4 = 1): one test each
BIG_CASES = {
    "trip2_fwd": functools.lru_cache(maxsize=None)(
        functools.partial(make_case, "trip2_fwd", 2731, 47, 33, seed=101, valid="random")),
    "trip2_bwd": functools.lru_cache(maxsize=None)(
        functools.partial(make_case, "trip2_bwd", 5479, 47, 33, seed=102, valid="random")),
}
MAPPER_CASES = [n for n in CASES if not n.startswith(("rays_trk", "trk_"))]
TRACKER_CASES = [n for n in CASES if n.startswith(("rays_trk", "trk_"))]


@functools.lru_cache(maxsize=None)
def solved(name):
    """(case, float64 reference, bounds) of a named case, computed once per process and shared."""
    case = (CASES.get(name) or BIG_CASES[name])()
    ref = reference(case)
    return case, ref, bounds(case, ref)
