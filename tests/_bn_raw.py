"""Driver and checks of the BatchNorm geometry tests (tests/test_bn_geometry_gpu.py): one forward +
backward through the raw ``_C`` bindings with an explicit ticket array (``run_raw``; also what the
knob tests' child processes run), and the layered assertions on what it returned (``check_raw``):
each pass against a float64 function of the previous pass's own outputs, so the bounds follow from
the arithmetic of that pass alone, then the whole against the full float64 model."""
from __future__ import annotations

import contextlib
import io
import math
from collections import namedtuple

import torch

from . import _norm_ref as R
from ._edge_ref import assert_by_measured_error, bf16_ulp_of

EPS, MOM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # eps as the kernels hold it

# relu, residual, mask bytes wanted, second gradient addend, residual gradient wanted,
# weight / bias present, running statistics present
Variant = namedtuple("Variant", "relu res want_mask dy2 want_dres affine running")


def vec(dtype) -> int:
    return 4 if dtype == torch.float32 else 8


# ----------------------------------------------------------------------------- launch geometry
K_RED, K_RED_BLOCKS, K_MAX_GX, K_WIDE_ROWS = 512, 384, 256, 262144


def geom(M, C, dtype, forced_tc=0, rpt=16, red_blocks=K_RED_BLOCKS):
    """Replica of batchnorm.hip's geom(): the reduction grid of an [M, C] tensor."""
    cv = C // vec(dtype)
    mt = forced_tc or (32 if M >= K_WIDE_ROWS else 8)
    tc = min(cv, mt)
    rpi = K_RED // tc
    gy = -(-cv // tc)
    want = -(-M // (rpi * rpt))
    cap = max(1, min(red_blocks // gy, K_MAX_GX))
    gx = max(1, min(want, cap))
    rows = -(-M // gx)
    gx = -(-M // rows)
    return dict(cv=cv, TC=tc, RPI=rpi, gy=gy, gx=gx, want=want, cap=cap, rows_per_block=rows,
                idle=K_RED - tc * rpi, P=K_RED // (tc * vec(dtype) // 4), last_tile=cv - (gy - 1) * tc)


def num_tickets(C, dtype, forced_tc=0) -> int:
    """One ticket per channel tile of the narrowest tile any M may get (bn_num_tickets)."""
    cv = C // vec(dtype)
    return -(-cv // min(cv, forced_tc or 8))


# ----------------------------------------------------------------------------- inputs
def make_inputs(M, C, dtype, seed, dev, gen_dev="cpu", shape4d=None):
    """Distinguishable channels: x[:, c] = (1 + c % 7) (randn +- 3) + (c % 61 - 30) / 4 (periods 7
    and 61: no two channels a tile width -- 32 to 256 -- apart look alike, and the means stay small
    enough for the fp32 end-to-end tolerance at any C; +3 on even rows, -3 on odd ones, so that a
    batch of two has a spread in every channel: two nearly equal samples mean invstd ~ 300, and no
    fp32 arithmetic holds an absolute tolerance there); weights of both signs in +-(0.5, 1.5), biases in
    (-0.5, 0.5); independent dy, dy2 and residual. ``shape4d`` (N, C, H, W): the same rows as a
    channels_last tensor."""
    g = torch.Generator(device=gen_dev).manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, generator=g, device=gen_dev)

    def unif(lo, hi):
        return torch.rand(C, generator=g, device=gen_dev) * (hi - lo) + lo

    c = torch.arange(C, device=gen_dev, dtype=torch.float32)

    def act(t):
        t = t.to(dtype).to(dev)
        if shape4d is not None:
            n, _, h, w = shape4d
            t = t.view(n, h, w, C).permute(0, 3, 1, 2)
            assert t.is_contiguous(memory_format=torch.channels_last)
        return t

    alt = 3.0 - 6.0 * (torch.arange(M, device=gen_dev) % 2).float()[:, None]
    inp = dict(x=act((randn(M, C) + alt) * (1 + c % 7) + 0.25 * (c % 61 - 30)))
    sign = torch.where(torch.rand(C, generator=g, device=gen_dev) < 0.5, -1.0, 1.0)
    inp["w"] = (unif(0.5, 1.5) * sign).to(dev)
    inp["b"] = unif(-0.5, 0.5).to(dev)
    inp["rm"], inp["rv"] = unif(-1.0, 1.0).to(dev), unif(0.5, 1.5).to(dev)
    for k in ("r", "dy", "dy2"):
        inp[k] = act(randn(M, C))
    return inp


# ----------------------------------------------------------------------------- the launches
def run_raw(nat, inp, v: Variant, forced_tc=0):
    """Every launch of one variant; returns the outputs (tensors on the GPU) and ``armed``: whether
    the ticket array was all zero after each launch."""
    x, dy = inp["x"], inp["dy"]
    dev, C = x.device, x.shape[1]
    w, b = (inp["w"], inp["b"]) if v.affine else (None, None)
    r = inp["r"] if v.res else None
    dy2 = inp["dy2"] if v.dy2 else None
    tk = torch.zeros(num_tickets(C, x.dtype, forced_tc), dtype=torch.int32, device=dev)
    o = {"armed": []}

    def launched():
        o["armed"].append(not bool(tk.any()))

    def buffers(zero):
        if zero:
            return torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
        return inp["rm"].clone(), inp["rv"].clone(), torch.zeros((), dtype=torch.int64, device=dev)

    rm, rv, nbt = buffers(False) if v.running else (None, None, None)
    y, st, mk = nat.bn_fwd_train(x, w, b, rm, rv, nbt, r, v.relu, MOM, EPS, tk, v.want_mask, False)
    launched()
    o.update(y=y, stats=st, mask=mk, rm=rm, rv=rv, nbt=nbt)
    # statistics only, momentum 1 into zeroed buffers: running_mean / running_var come back as the
    # mean and the unbiased variance the kernel holds, rounded once to float
    rm1, rv1, nbt1 = buffers(True)
    y0, st0, mk0 = nat.bn_fwd_train(x, w, b, rm1, rv1, nbt1, None, v.relu, 1.0, EPS, tk, False, True)
    launched()
    assert y0 is None and mk0 is None
    o.update(stats_so=st0, mean1=rm1, uvar1=rv1, nbt1=nbt1)
    o["y_apply"], o["mask_apply"] = nat.bn_fwd_apply(x, st, r, v.relu, v.want_mask)
    o["y_bnapply"] = nat.bn_apply(x, r, st[2], st[3], v.relu)

    def bwd(want_dres, y_src, mask_src, dw_out=None, db_out=None):
        out = nat.bn_bwd(dy, x, y_src, w, st, v.relu, want_dres, True, tk, dw_out, db_out, dy2, mask_src)
        launched()
        return out

    # R1, the variant's own call with the mask source the module would use: the mask bytes where
    # the forward wrote them (they need want_dres), else y, else recomputed from x (no residual)
    if not v.relu:
        ys, ms = None, None
    elif mk is not None and v.want_dres:
        ys, ms = None, mk
    elif v.res or v.want_dres:
        ys, ms = y, None
    else:
        ys, ms = None, None
    o["r1_dx"], o["r1_dw"], o["r1_db"], o["r1_dres"] = bwd(v.want_dres, ys, ms)
    # R2: the residual gradient wanted, the mask from y, the parameter gradients written in place
    dw_out, db_out = torch.full((C,), math.nan, device=dev), torch.full((C,), math.nan, device=dev)
    o["r2_dx"], dw2, db2, o["r2_dres"] = bwd(True, y if v.relu else None, None, dw_out, db_out)
    o["r2_dw"], o["r2_db"] = dw_out, db_out
    o["r2_alias"] = dw2.data_ptr() == dw_out.data_ptr() and db2.data_ptr() == db_out.data_ptr()
    # R3: the reduce pass and the g-based apply pass as a pair (mask bytes, or recomputed from x)
    if not (v.relu and v.res and mk is None):
        o["r3_g"], o["r3_dw"], o["r3_db"], o["coef"] = nat.bn_bwd_reduce(dy, x, w, st, v.relu, True, tk, None, None,
                                                                        dy2, mk)
        launched()
        o["r3_dx"] = nat.bn_bwd_apply_g(o["r3_g"], x, o["coef"])
    return o


def to_cpu(o):
    return {k: (t.cpu() if isinstance(t, torch.Tensor) else t) for k, t in o.items()}


def same_bits(a, b):
    """Two runs' outputs are bit-identical."""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), f"{k} differs between two identical launches"
        else:
            assert a[k] == b[k], k


# ----------------------------------------------------------------------------- the checks
def ulp32(v64):
    """Spacing of fp32 numbers at |v|."""
    return torch.exp2(torch.floor(torch.log2(v64.abs().clamp_min(2.0 ** -126))) - 23)


def _within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the derived bound, worst "
                           f"error / bound = {float((err / bound.clamp_min(1e-300))[bad].max()):.3f}")


def _measured(got, torch32, ref64, what, loud):
    """assert_by_measured_error with the floor of one rounding of the float64 value to the stored
    float; ``loud`` False keeps its [measured] line out of the output (the rule is the same)."""
    ref64 = ref64.detach().cpu()
    floor = 2.0 ** -23 * float(ref64.abs().max())
    with contextlib.nullcontext() if loud else contextlib.redirect_stdout(io.StringIO()):
        return assert_by_measured_error(got.detach().cpu(), torch32.detach().cpu(), ref64, floor=floor, what=what)


class Case:
    """What every variant of one input set shares: the float64 rows and the float64 statistics."""

    def __init__(self, inp, ref_dev):
        self.inp, self.dev = inp, torch.device(ref_dev)
        self.dtype = inp["x"].dtype
        self.X32 = self.rows32(inp["x"])
        self.X = self.X32.double()
        self.M, self.C = self.X.shape
        self.w, self.b = self.f64(inp["w"]), self.f64(inp["b"])
        self.stats = {a: R.bn_stats_ref(self.X, self.w if a else None, self.b if a else None, EPS32)
                      for a in (True, False)}
        self.var32, self.mean32 = torch.var_mean(self.X32, dim=0, unbiased=False)
        self.measured = set()  # quantities whose [measured] line has been printed

    def f64(self, t):
        return t.detach().to(self.dev, torch.float64)

    def rows32(self, t):
        t = t.detach().to(self.dev)
        if t.dim() == 4:
            t = t.permute(0, 2, 3, 1)
        return t.reshape(-1, t.shape[-1]).float()

    def rows(self, t):
        return self.rows32(t).double()

    def loud(self, key):
        first = key not in self.measured
        self.measured.add(key)
        return first


def check_raw(case: Case, v: Variant, o, tag):
    inp, M, C, X, X32 = case.inp, case.M, case.C, case.X, case.X32
    bf = case.dtype == torch.bfloat16
    V = vec(case.dtype)
    f64, rows = case.f64, case.rows
    w = case.w if v.affine else torch.ones_like(case.w)
    b = case.b if v.affine else torch.zeros_like(case.b)
    Rr = rows(inp["r"]) if v.res else None
    mean, var, invstd, scale, shift = case.stats[v.affine]

    def half_ulp(ref):
        return 0.5 * bf16_ulp_of(ref) if bf else torch.zeros_like(ref)

    # ---- hand-off: every launch re-armed its tickets; in-place parameter gradients
    assert all(o["armed"]) and len(o["armed"]) >= 4, f"{tag}: tickets not re-armed after launch {o['armed']}"
    assert o["r2_alias"], f"{tag}: dweight_out / dbias_out not returned as the gradients"

    # ---- statistics
    assert torch.equal(o["stats"], o["stats_so"]), f"{tag}: stats_only statistics differ from the full call's"
    mean_k, invstd_k, scale_k, shift_k = f64(o["stats"])
    assert torch.equal(o["mean1"], o["stats"][0])
    assert int(o["nbt1"]) == 1
    var_k = f64(o["uvar1"]) * ((M - 1) / M if M > 1 else 1.0)
    _measured(mean_k, case.mean32, mean, f"{tag} mean", case.loud("mean"))
    _measured(var_k, case.var32, var, f"{tag} var", case.loud("var"))
    inv_from_k = 1.0 / torch.sqrt(var_k + EPS32)
    _within(invstd_k, inv_from_k, 2 * ulp32(inv_from_k), f"{tag} invstd from the kernel's var")
    _within(scale_k, w * invstd_k, 2 * ulp32(w * invstd_k), f"{tag} scale")
    ms = mean_k * w * invstd_k
    _within(shift_k, b - ms, 2 * ulp32(b.abs() + ms.abs()), f"{tag} shift")
    if v.running:
        rm_ref, rv_ref = R.bn_running_ref(mean, var, M, f64(inp["rm"]), f64(inp["rv"]), MOM)
        torch.testing.assert_close(f64(o["rm"]), rm_ref, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(f64(o["rv"]), rv_ref, rtol=1e-4, atol=1e-5)
        assert int(o["nbt"]) == 1
    if M == 1:
        assert torch.equal(o["stats"][1], torch.full_like(o["stats"][1], 1.0 / math.sqrt(EPS32)))
        assert not var_k.any()

    # ---- apply, from the kernel's own scale / shift
    Y = rows(o["y"])
    pre = X * scale_k + shift_k
    bound = 2.0 ** -22 * ((X * scale_k).abs() + shift_k.abs())
    if v.res:
        pre, bound = pre + Rr, bound + 2.0 ** -22 * Rr.abs()
    y_ref = pre.clamp_min(0.0) if v.relu else pre
    _within(Y, y_ref, bound + half_ulp(y_ref), f"{tag} y from the kernel's scale/shift")
    assert torch.equal(o["y"], o["y_apply"]), f"{tag}: bn_fwd_apply differs from bn_fwd_train"
    assert torch.equal(o["y"], o["y_bnapply"]), f"{tag}: bn_apply differs from bn_fwd_train"
    if v.relu and v.res and v.want_mask:
        bits = ((Y.view(M, C // V, V) > 0).to(torch.int64) << torch.arange(V, device=case.dev)).sum(-1)
        assert torch.equal(o["mask"].to(case.dev).view(M, C // V).to(torch.int64), bits), f"{tag}: mask != bits of y > 0"
        assert torch.equal(o["mask"], o["mask_apply"])
    else:
        assert o["mask"] is None and o["mask_apply"] is None
    if M == 1:  # one row: y is the bias (+ residual), to the apply bound and shift's own rounding
        target = b + (Rr if v.res else 0.0)
        target = target.clamp_min(0.0) if v.relu else target
        _within(Y, target.expand_as(Y), bound + 2 * ulp32(b.abs() + ms.abs()) + half_ulp(y_ref), f"{tag} y at M = 1")

    # ---- backward reduce. The mask is the kernel's own forward's (y > 0, proven above); the
    # masked gradient is then exact arithmetic: one IEEE add of dy2 in fp32, one rounding to the
    # tensor's type where it is materialised
    pos = (Y > 0) if v.relu else torch.ones_like(Y, dtype=torch.bool)
    g32 = case.rows32(inp["dy"])
    if v.dy2:
        g32 = g32 + case.rows32(inp["dy2"])
    g32 = g32 * pos
    G = g32.to(case.dtype).double()  # what the reduce pass writes (GOUT) and sums
    assert torch.equal(rows(o["r2_dres"]), G), f"{tag}: dres is not mask * (dy + dy2) rounded once"
    sdy, sdx = G.sum(0), (G * (X - mean_k)).sum(0)
    G32 = G.float()
    db32 = G32.sum(0)
    dw32 = (G32 * (X32 - mean_k.float())).sum(0) * invstd_k.float()
    _measured(f64(o["r2_db"]), db32, sdy, f"{tag} dbias", case.loud("dbias"))
    _measured(f64(o["r2_dw"]), dw32, sdx * invstd_k, f"{tag} dweight", case.loud("dweight"))
    if "coef" in o:
        for k in ("dw", "db", "dx"):
            assert torch.equal(o["r3_" + k], o["r2_" + k]), f"{tag}: bn_bwd_reduce + apply_g {k} != bn_bwd"
        assert torch.equal(o["r3_g"], o["r2_dres"]), f"{tag}: bn_bwd_reduce g != bn_bwd dres"
        A_k, B_k, C_k = f64(o["coef"])
        kk = w * invstd_k
        s1 = f64(o["r3_db"]) / M
        s2 = invstd_k * f64(o["r3_dw"]) / M  # dweight = invstd * sum g (x - mean)
        _within(A_k, kk, 4 * ulp32(kk), f"{tag} coef A")
        _within(B_k, -kk * s2, 4 * ulp32(kk * s2), f"{tag} coef B")
        _within(C_k, kk * s2 * mean_k - kk * s1, 4 * ulp32((kk * s2 * mean_k).abs() + (kk * s1).abs()),
                f"{tag} coef C")
        # ---- backward apply, from the kernel's own coefficients: two fmas
        dx_ref = A_k * G + B_k * X + C_k
        dbound = 2.0 ** -22 * ((A_k * G).abs() + (B_k * X).abs() + C_k.abs())
        _within(rows(o["r2_dx"]), dx_ref, dbound + half_ulp(dx_ref), f"{tag} dx from the kernel's coefficients")
        if M == 1:
            _within(rows(o["r2_dx"]), torch.zeros_like(dx_ref), dbound + half_ulp(dx_ref), f"{tag} dx at M = 1")
    # the variant's own call against R2: same mask, same g unless bf16 sums the unrounded dy + dy2
    if v.want_dres:
        assert torch.equal(o["r1_dres"], o["r2_dres"]), f"{tag}: dres differs between mask sources"
    else:
        assert o["r1_dres"] is None
    if v.want_dres or not (bf and v.dy2):
        for k in ("dx", "dw", "db"):
            assert torch.equal(o["r1_" + k], o["r2_" + k]), f"{tag}: {k} differs between mask sources / dres paths"

    # ---- end to end, at the tolerances of test_native_bn_train_fwd_bwd, no element left out
    if M > 1:
        tol = 2e-2 if bf else 2e-5
        gtol = 5e-2 if bf else 1e-4
        wtol = 1e-3 * M ** 0.5 if bf else 1e-3
        _, y_full = R.bn_apply_ref(X, scale, shift, Rr, v.relu)
        torch.testing.assert_close(Y, y_full, rtol=tol, atol=tol)
        # the gradient the backward is OF: where the residual gradient is materialised (want_dres) it
        # is mask * (dy + dy2) as the tensor's type holds it -- the sums use that rounded g, so both
        # passes agree --, else the fp32 sum; each proven above to be the right rounding of the exact one
        exact = (rows(inp["dy"]) + rows(inp["dy2"]) if v.dy2 else rows(inp["dy"])) * pos
        torch.testing.assert_close(rows(o["r2_dres"]), exact, rtol=gtol, atol=gtol)
        for run, g in (("r1", G if v.want_dres else g32.double()), ("r2", G)):
            db_f, dw_f, _, _, _, dx_f = R.bn_backward_ref(g, X, mean, invstd, w, M)
            torch.testing.assert_close(rows(o[run + "_dx"]), dx_f, rtol=gtol, atol=gtol)
            torch.testing.assert_close(f64(o[run + "_dw"]), dw_f, rtol=1e-3, atol=wtol)
            torch.testing.assert_close(f64(o[run + "_db"]), db_f, rtol=1e-3, atol=wtol)


# ----------------------------------------------------------------------------- variant sets
_FWD = [(False, False, False), (False, True, False), (True, False, False), (True, True, False), (True, True, True)]


def full_cross():
    """relu x residual x mask bytes, x dy2, x want_dres, x affine, x running statistics."""
    return [Variant(relu, res, wm, dy2, dres, aff, run)
            for aff in (True, False) for run in (True, False) for relu, res, wm in _FWD
            for dy2 in (False, True) for dres in (False, True)]


# every mask source and both backward apply kernels once: mask bytes + dy2 + dres; the mask
# recomputed from x, no buffers; no ReLU, no affine, dy2 summed unrounded; the mask from y
REDUCED = [Variant(True, True, True, True, True, True, True), Variant(True, False, False, False, False, True, False),
           Variant(False, True, False, True, False, False, True), Variant(True, True, False, False, True, True, True)]

# what the knob tests' child processes run (shapes by dtype name: the child gets them from here)
KNOB_SEED = 23
KNOB_SHAPES = [("bfloat16", 1000, 72), ("bfloat16", 4099, 160), ("float32", 4099, 80), ("float32", 777, 520)]
KNOB_VARIANTS = REDUCED
