"""Float64 reference of along-ray occupancy compositing (csrc/composite.hip; oracle/render_math.raw2nerf_color and the logit
composite sum_s w_s logits_s) with hand-written gradients, and the seeded occupancy regimes of a TRAINED scene the tests feed it:
surfaces where sigmoid(10 occ) rounds to exactly 1, transmittance that steps down by 1e-10 per opaque sample into underflow,
nearly empty rays.  CPU only.

fp32 cannot represent 1 - alpha once alpha >= 1 - 2^-24, so a float64 sigmoid would describe another function than any fp32
implementation computes.  The reference therefore starts from alpha = fp32(sigmoid(10 occ)) (sigmoid evaluated in float64, rounded
once) and is float64 from there on, including d_occ = 10 a (1 - a) dL/da at that same a.  It is evaluated at that alpha and with
EVERY alpha moved to its fp32 neighbour above / below (clamped to [0, 1]); `spread` is the larger element-wise deviation of the two
from the centre -- the sensitivity of the operation itself to one ulp of alpha.  An implementation is held to

    |got - ref| <= 1e-5 |ref| + 1e-6 scale + 4 spread        (bound())

scale = max |ref| of the tensor (for d_occ: at least 10 max_s |dL/dw_s| of the ray -- a one-sample ray has an exactly zero gradient);
the factor 4 lets expf and the division of an fp32 sigmoid land two ulps from the correctly rounded alpha on either side.
"""
import numpy as np
import torch

OUT_KEYS = ("depth", "var", "rgb", "weights", "sem", "d_raw", "d_logits")


def alpha32(occ: torch.Tensor) -> torch.Tensor:
    """fp32(sigmoid(10 occ)), the sigmoid in float64; returned as float64."""
    return torch.sigmoid(10.0 * occ.double()).float().double()


def _neighbour(a64: torch.Tensor, up: bool) -> torch.Tensor:
    a = a64.float().numpy()
    b = np.nextafter(a, np.float32(2.0 if up else -1.0))
    return torch.from_numpy(np.clip(b, np.float32(0.0), np.float32(1.0))).double()


def _eval(alpha, rgb_in, z, logits, grads, rgb_logits):
    """Everything in float64 from a given alpha [N, S].  grads: dict with depth [N], var [N], rgb [N, 3], weights [N, S], sem [N, C]
    (missing / None = no gradient from that output)."""
    N, S = alpha.shape
    col = torch.sigmoid(rgb_in) if rgb_logits else rgb_in
    om = (1.0 - alpha) + 1e-10
    T = torch.cumprod(torch.cat((torch.ones(N, 1, dtype=torch.float64), om), -1), -1)[:, :-1]
    u = alpha * T
    sumu = u.sum(-1, keepdim=True)
    w = u / sumu                                                       # no epsilon: an all-dead ray is 0 / 0 = NaN (D9)
    depth = (w * z).sum(-1)
    t = z - depth[:, None]
    var = (w * t * t).sum(-1)
    rgb = (w[..., None] * col).sum(-2)
    sem = (w[..., None] * logits).sum(-2) if logits is not None else torch.zeros(N, 0, dtype=torch.float64)
    out = {"depth": depth, "var": var, "rgb": rgb, "weights": w, "sem": sem}
    if grads is None:
        return out
    zero = lambda *s: torch.zeros(*s, dtype=torch.float64)
    gD = grads.get("depth") if grads.get("depth") is not None else zero(N)
    gV = grads.get("var") if grads.get("var") is not None else zero(N)
    gC = grads.get("rgb") if grads.get("rgb") is not None else zero(N, 3)
    gW = grads.get("weights") if grads.get("weights") is not None else zero(N, S)
    gS = grads.get("sem") if (grads.get("sem") is not None and logits is not None) else None
    # G_s = dL/dw_s with w free; var also moves through depth: d var / d depth = -2 sum w (z - depth) (zero once sum w = 1)
    gDv = gD + gV * (-2.0) * (w * t).sum(-1)
    G = (gC[:, None, :] * col).sum(-1) + gDv[:, None] * z + gV[:, None] * t * t + gW
    if gS is not None:
        G = G + (gS[:, None, :] * logits).sum(-1)
    du = (G - (w * G).sum(-1, keepdim=True)) / sumu                    # dL/du_s through w = u / sum u
    k = du * u
    # sum_{j > s} du_j u_j (every T_j, j > s, holds the factor om_s): an exclusive suffix sum, formed without subtracting k_s back out
    # -- the quotient by om = 1e-10 would magnify that cancellation
    incl = torch.flip(torch.cumsum(torch.flip(k, (-1,)), -1), (-1,))
    later = torch.cat((incl[:, 1:], torch.zeros(N, 1, dtype=torch.float64)), -1)
    dalpha = du * T - later / om
    d_raw = torch.empty(N, S, 4, dtype=torch.float64)
    d_col = w[..., None] * gC[:, None, :]
    d_raw[..., :3] = d_col * col * (1.0 - col) if rgb_logits else d_col
    d_raw[..., 3] = 10.0 * alpha * (1.0 - alpha) * dalpha
    out["d_raw"] = d_raw
    if logits is not None:
        out["d_logits"] = w[..., None] * gS[:, None, :] if gS is not None else torch.zeros_like(logits)
    else:
        out["d_logits"] = torch.zeros(N, S, 0, dtype=torch.float64)
    out["G"] = G
    return out


def composite64(raw, z, logits=None, grads=None, rgb_logits=False, pure=False):
    """-> (ref, spread): dicts of float64 tensors over OUT_KEYS (the gradient keys only with `grads`).  raw [N, S, 4] (colour or, with
    rgb_logits, colour logits; occupancy last), z [N, S], logits [N, S, C] or None; fp32 or float64 inputs.  pure: alpha is the
    float64 sigmoid itself (no fp32 rounding; spread is then zero) -- for reporting how far fp32's alpha is from the real function."""
    raw, z = raw.detach().double(), z.detach().double()
    logits = logits.detach().double() if logits is not None and logits.shape[-1] > 0 else None
    grads = None if grads is None else {k: (None if v is None else v.detach().double()) for k, v in grads.items()}
    occ = raw[..., 3]
    if pure:
        ref = _eval(torch.sigmoid(10.0 * occ), raw[..., :3], z, logits, grads, rgb_logits)
        return ref, {k: torch.zeros_like(v) for k, v in ref.items()}
    a = alpha32(occ)
    ref = _eval(a, raw[..., :3], z, logits, grads, rgb_logits)
    hi = _eval(_neighbour(a, True), raw[..., :3], z, logits, grads, rgb_logits)
    lo = _eval(_neighbour(a, False), raw[..., :3], z, logits, grads, rgb_logits)
    spread = {}
    for k, v in ref.items():
        s = torch.maximum((hi[k] - v).abs(), (lo[k] - v).abs())
        spread[k] = torch.where(torch.isfinite(s), s, torch.zeros_like(s))   # (only where the centre is finite is anything bounded)
    return ref, spread


def bound(key, ref, spread):
    """The element-wise tolerance of output `key` (see the module docstring)."""
    r = ref[key]
    fin = torch.isfinite(r)
    scale = r[fin].abs().max() if bool(fin.any()) else torch.zeros((), dtype=torch.float64)
    tol = 1e-5 * r.abs() + 1e-6 * scale + 4.0 * spread[key]
    if key == "d_raw":
        G = ref["G"]
        gmax = torch.where(torch.isfinite(G), G.abs(), torch.zeros_like(G)).amax(-1, keepdim=True)      # per ray
        occ_scale = torch.maximum(scale.expand_as(gmax), 10.0 * gmax)
        tol[..., 3] = 1e-5 * r[..., 3].abs() + 1e-6 * occ_scale + 4.0 * spread[key][..., 3]
    return tol


def worst_ratio(key, got, ref, spread):
    """max |got - ref| / bound over the entries where the reference is finite; inf if a NaN / Inf is not where the reference has it."""
    r = ref[key]
    got = got.detach().double().cpu().reshape(r.shape)
    if r.numel() == 0:
        return 0.0
    if not (torch.equal(torch.isnan(got), torch.isnan(r)) and torch.equal(torch.isinf(got), torch.isinf(r))):
        return float("inf")
    fin = torch.isfinite(r)
    if not bool(fin.any()):
        return 0.0
    d = (got - r).abs()[fin]
    tol = bound(key, ref, spread)[fin]
    return float(torch.where(d == 0, torch.zeros_like(d), d / tol.clamp_min(1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------- inputs
REGIMES = ("mild", "surface", "sat", "edge", "faint", "late", "walls")
S_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)      # around the 1 / 2 / 4 samples-per-lane switches at S = 64 and 128

_CASES = {}


def case(regime: str, N: int, S: int, C: int, rgb_logits: bool = False):
    """Seeded inputs and output gradients of one regime, fp32 on the CPU, built once per session:
    dict(raw, z, logits (None when C = 0), grads)."""
    key = (regime, N, S, C, rgb_logits)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + 7 * N + 13 * S + C + (500 if rgb_logits else 0))
    rnd = lambda *s: torch.randn(*s, generator=g)
    uni = lambda *s: torch.rand(*s, generator=g)
    raw = torch.empty(N, S, 4)
    raw[..., :3] = rnd(N, S, 3) if (rgb_logits or regime == "mild") else uni(N, S, 3)
    z = torch.sort(uni(N, S) * 4 + 0.1, -1)[0]
    if regime == "mild":                                   # the inputs of test_composite_vs_oracle
        occ = rnd(N, S) * 0.3
    elif regime == "surface":                              # free space, then a surface from a random sample on
        first = torch.randint(0, S, (N, 1), generator=g)
        behind = torch.arange(S)[None, :] >= first
        occ = torch.where(behind, 2.0 + uni(N, S), -2.0 + 0.1 * rnd(N, S))
    elif regime == "sat":
        occ = torch.full((N, S), 3.0)
    elif regime == "edge":                                 # alpha rounds to 1 or to 1 - 2^-24
        occ = 1.6 + 0.3 * uni(N, S)
    elif regime == "faint":                                # sum u is small and the division by it amplifies
        occ = -1.5 + 0.05 * rnd(N, S)
    elif regime == "late":
        occ = torch.full((N, S), -3.0)
        occ[:, -1] = 0.3 + 0.2 * uni(N)
    elif regime == "walls":                                # T steps through 1e-10, 1e-20, ... and into underflow
        occ = -2.0 + 0.1 * rnd(N, S)
        occ[:, 3::7] = 4.0
    else:
        raise KeyError(regime)
    raw[..., 3] = occ
    logits = rnd(N, S, C) if C else None
    grads = {"depth": rnd(N), "var": rnd(N), "rgb": rnd(N, 3), "weights": rnd(N, S), "sem": rnd(N, C) if C else None}
    _CASES[key] = dict(raw=raw, z=z, logits=logits, grads=grads)
    return _CASES[key]


_REFS = {}


def reference(regime, N, S, C, rgb_logits=False, only=None):
    """composite64 of case(...), computed once per session.  only: a tuple of gradient keys to keep (the others are None)."""
    key = (regime, N, S, C, rgb_logits, only)
    if key not in _REFS:
        cs = case(regime, N, S, C, rgb_logits)
        grads = cs["grads"] if only is None else {k: (v if k in only else None) for k, v in cs["grads"].items()}
        _REFS[key] = composite64(cs["raw"], cs["z"], cs["logits"], grads, rgb_logits)
    return _REFS[key]
