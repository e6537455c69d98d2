"""The NHWC BatchNorm kernels (csrc/kernels/batchnorm.hip) at the edges of their launch geometry,
through the raw bindings with an explicit ticket array: partial and odd channel tiles, the wide
tile, both row-block caps, every mask source, the cross-rank instances, the environment knobs (in
child processes) and channel counts whose per-channel tables pass 64 KiB of LDS. The launches and
the layered assertions live in tests/_bn_raw.py, the float64 model in tests/_norm_ref.py."""
import math
import os
import subprocess
import sys

import pytest
import torch

from . import _bn_raw as B
from . import _norm_ref as R
from ._edge_ref import assert_by_measured_error

F32, BF16 = torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(case):
    dt, M, C = case
    return f"{'f32' if dt == F32 else 'bf16'}-{M}x{C}"


# the smallest shape that reaches each path (B.geom, a replica of the kernels' geom(), says so below)
SMALL = ([(F32, 513, 4), (BF16, 513, 8)]                                     # one vector per row
         + [(F32, 333, 12), (F32, 333, 20), (F32, 333, 28)]                  # TC 3 / 5 / 7: idle threads
         + [(BF16, 333, 24), (BF16, 333, 40), (BF16, 333, 56)]
         + [(F32, 1000, 36), (BF16, 1000, 72)]                               # partial last tile (1 vector)
         + [(F32, m, 64) for m in (1, 2, 63, 64, 65, 511, 513, 1023, 1025)]  # unroll tails, gx 1 -> 2
         + [(BF16, 8193, 64)])                                               # gx 9, short tail block
TALL = [(BF16, 12291, 2048), (F32, 6200, 2048),      # row blocks capped by the channel tiles
        (BF16, 2 ** 21 + 4097, 8),                   # kMaxGx clamp
        (BF16, 262143, 256), (BF16, 262144, 256),    # either side of the wide tile
        (BF16, 262144, 320), (F32, 262147, 144)]     # wide tile with a partial last tile


def test_shapes_reach_the_paths_they_are_named_for():
    g = lambda dt, M, C: B.geom(M, C, dt)  # noqa: E731
    for dt, C in ((F32, 4), (BF16, 8)):
        assert (g(dt, 513, C)["TC"], g(dt, 513, C)["RPI"]) == (1, 512)
    for dt, v in ((F32, 4), (BF16, 8)):
        assert [(g(dt, 333, t * v)["TC"], g(dt, 333, t * v)["idle"]) for t in (3, 5, 7)] == [(3, 2), (5, 2), (7, 1)]
        e = g(dt, 1000, 9 * v)
        assert (e["cv"], e["gy"], e["last_tile"]) == (9, 2, 1)
    assert (g(F32, 333, 20)["P"], g(F32, 333, 28)["P"]) == (102, 73)
    assert g(F32, 1023, 64)["gx"] == 1 and g(F32, 1025, 64)["gx"] == 2
    assert (g(BF16, 8193, 64)["gx"], g(BF16, 8193, 64)["rows_per_block"]) == (9, 911)
    for dt, M, gy, want, cap in ((BF16, 12291, 32, 13, 12), (F32, 6200, 64, 7, 6)):
        e = g(dt, M, 2048)
        assert (e["gy"], e["want"], e["cap"], e["gx"]) == (gy, want, cap, cap)
    e = g(BF16, 2 ** 21 + 4097, 8)
    assert e["want"] == 257 and e["gx"] == B.K_MAX_GX
    assert (g(BF16, 262143, 256)["TC"], g(BF16, 262143, 256)["gy"]) == (8, 4)
    e = g(BF16, 262144, 256)
    assert (e["TC"], e["gy"], e["gx"]) == (32, 1, 256)
    assert [(g(dt, M, C)["TC"], g(dt, M, C)["gy"], g(dt, M, C)["last_tile"])
            for dt, M, C in TALL[5:]] == [(32, 2, 8), (32, 2, 4)]


@pytest.mark.gpu
def test_geometry_replica_is_the_kernels(native):
    """B.geom / B.num_tickets, which pick the shapes above, against the geometry the launches use."""
    knob = [(getattr(torch, dt), M, C) for dt, M, C in B.KNOB_SHAPES]
    for dt, M, C in SMALL + TALL + knob + [(F32, 64, 8192), (BF16, 64, 8192), (BF16, 128 * 56 * 56, 64)]:
        e = B.geom(M, C, dt)
        tc, rpi, gx, gy, ws, tickets = native.bn_geometry(M, C, dt == F32)
        assert (tc, rpi, gx, gy) == (e["TC"], e["RPI"], e["gx"], e["gy"]), (dt, M, C)
        assert ws == 2 * e["gx"] * C and tickets == B.num_tickets(C, dt), (dt, M, C)


def _run_and_check(native, dev, dtype, M, C, variants, tall=False, shape4d=None):
    seed = M * 7 + C
    inp = B.make_inputs(M, C, dtype, seed, dev, gen_dev=dev if tall else "cpu", shape4d=shape4d)
    case = B.Case(inp, dev if tall else "cpu")
    tag = _id((dtype, M, C))
    for i, v in enumerate(variants):
        o = B.run_raw(native, inp, v)
        B.same_bits(o, B.run_raw(native, inp, v))  # a second identical launch: identical bits
        B.check_raw(case, v, o, f"{tag} {tuple(int(f) for f in v)}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL, ids=_id)
def test_bn_small_shapes_full_cross(native, dev, case):
    dtype, M, C = case
    _run_and_check(native, dev, dtype, M, C, B.full_cross())


@pytest.mark.gpu
@pytest.mark.parametrize("case", TALL, ids=_id)
def test_bn_tall_shapes(native, dev, case):
    """The float64 reference of these runs on the GPU in plain torch float64 ops."""
    dtype, M, C = case
    _run_and_check(native, dev, dtype, M, C, B.REDUCED, tall=True)


@pytest.mark.gpu
def test_bn_channels_last_4d_is_the_rows_view(native, dev):
    _run_and_check(native, dev, BF16, 3 * 5 * 7, 72, B.full_cross(), shape4d=(3, 72, 5, 7))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,C", [(F32, 36), (BF16, 72), (F32, 2048), (BF16, 64)])
def test_bn_tickets_one_short_raise(native, dev, dtype, C):
    x = torch.randn(64, C, device=dev).to(dtype)
    need = B.num_tickets(C, dtype)
    # a view one element short of a longer zeroed buffer: were the check ever to let it through,
    # the kernels' tickets would still land in memory this test owns
    short = torch.zeros(need + 63, dtype=torch.int32, device=dev)[:need - 1]
    st = torch.zeros(4, C, device=dev)
    with pytest.raises(RuntimeError, match="tickets"):
        native.bn_fwd_train(x, None, None, None, None, None, None, False, 0.1, 1e-5, short, False, False)
    with pytest.raises(RuntimeError, match="tickets"):
        native.bn_bwd(x, x, None, None, st, False, False, True, short, None, None, None, None)
    with pytest.raises(RuntimeError, match="tickets"):
        native.bn_sync_stats(x, torch.zeros(2 * C + 1, dtype=torch.float64, device=dev), short)
    exact = torch.zeros(need, dtype=torch.int32, device=dev)
    native.bn_fwd_train(x, None, None, None, None, None, None, False, 0.1, 1e-5, exact, False, False)
    assert not exact.any()


@pytest.mark.gpu
def test_bn_bwd_residual_gradient_needs_the_forwards_mask(native, dev):
    """relu + want_dres with neither y nor the mask bytes would recompute the mask from x alone,
    which is wrong whenever a residual was added: the binding refuses it."""
    x = torch.randn(64, 32, device=dev)
    tk = torch.zeros(1, dtype=torch.int32, device=dev)
    y, st, _ = native.bn_fwd_train(x, None, None, None, None, None, x, True, 0.1, 1e-5, tk, False, False)
    with pytest.raises(RuntimeError, match="needs the forward's y or mask"):
        native.bn_bwd(x, x, None, None, st, True, True, True, tk, None, None, None, None)
    native.bn_bwd(x, x, y, None, st, True, True, True, tk, None, None, None, None)
    native.bn_bwd(x, x, None, None, st, True, False, True, tk, None, None, None, None)  # no residual: from x
    native.bn_bwd(x, x, None, None, st, False, True, True, tk, None, None, None, None)  # no ReLU: no mask


# ----------------------------------------------------------------------------- cross-rank instances
SYNC = [(BF16, 1000, 72), (F32, 1000, 36), (BF16, 333, 40), (F32, 333, 28), (BF16, 2 ** 21 + 4097, 8),
        (BF16, 262144, 320), (F32, 262147, 144)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SYNC, ids=_id)
def test_bn_sync_instances_on_uneven_chunks(native, dev, case):
    """bn_sync_stats / bn_sync_merge / bn_sync_bwd_reduce / bn_sync_coef on one GPU: the rows split
    into uneven "ranks", one of them without rows, against the sync_*_ref models."""
    dtype, M, C = case
    tall = M * C > 1_000_000
    inp = B.make_inputs(M, C, dtype, M + C, dev, gen_dev=dev if tall else "cpu")
    c = B.Case(inp, dev if tall else "cpu")
    tag, V, bf = _id(case), B.vec(dtype), dtype == BF16
    f64, X, X32 = c.f64, c.X, c.X32
    sizes = [M // 2 + 3, 0, 1, M - M // 2 - 4]
    bounds = [(sum(sizes[:i]), sum(sizes[:i + 1])) for i in range(len(sizes))]
    tk = torch.zeros(B.num_tickets(C, dtype), dtype=torch.int32, device=dev)
    recs = []
    for i, (a, e) in enumerate(bounds):
        rec = torch.zeros(2 * C + 1, dtype=torch.float64, device=dev)
        if e > a:
            rec.fill_(math.nan)
            native.bn_sync_stats(inp["x"][a:e], rec, tk)
            assert not tk.any()
            mean, m2, n = R.sync_record_ref(X[a:e])
            got = f64(rec)
            assert float(got[2 * C]) == n
            spread = mean.abs() + torch.sqrt(m2 / n)
            # rtol 1e-6 of |mean| + std, not of |mean| alone: the record's mean is K + s / n with s a
            # float sum of deviations of the size of std, so its error scales with std and a channel
            # whose mean is near 0 (c % 61 == 30 here) has no relative accuracy to speak of
            e_t = float((X32[a:e].mean(0).double() - mean).abs().max())
            print(f"[measured] {tag} record {i} mean: torch_fp32_err={e_t:.3e} "
                  f"kernel_err={float((got[:C] - mean).abs().max()):.3e} "
                  f"bound/std={1e-6:.0e} worst err/std={float(((got[:C] - mean).abs() / torch.sqrt(m2 / n).clamp_min(1e-30)).max()) if n > 1 else 0.0:.3e}")
            B._within(got[:C], mean, 1e-6 * spread, f"{tag} record {i} mean (rtol 1e-6 of |mean| + std)")
            t32 = ((X32[a:e] - X32[a:e].mean(0)) ** 2).sum(0)
            B._measured(got[C:2 * C], t32, m2, f"{tag} record M2", c.loud("m2"))
        recs.append(rec)
    gathered = torch.stack(recs)
    rm, rv = inp["rm"].clone(), inp["rv"].clone()
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    stats, count = native.bn_sync_merge(gathered, inp["w"], inp["b"], rm, rv, nbt, B.MOM, B.EPS)
    assert float(count) == M and int(nbt) == 1
    mean_m, m2_m, n = R.sync_merge_ref([(f64(r[:C]), f64(r[C:2 * C]), float(r[2 * C])) for r in recs])
    mean_k, invstd_k, scale_k, shift_k = f64(stats)
    inv = 1.0 / torch.sqrt(m2_m / n + B.EPS32)
    B._within(mean_k, mean_m, B.ulp32(mean_m), f"{tag} merged mean")
    B._within(invstd_k, inv, 2 * B.ulp32(inv), f"{tag} merged invstd")
    B._within(scale_k, c.w * invstd_k, 2 * B.ulp32(c.w * invstd_k), f"{tag} merged scale")
    ms = mean_k * c.w * invstd_k
    B._within(shift_k, c.b - ms, 2 * B.ulp32(c.b.abs() + ms.abs()), f"{tag} merged shift")
    mean, var, invstd, scale, shift = c.stats[True]
    rm_ref, rv_ref = R.bn_running_ref(mean, var, M, f64(inp["rm"]), f64(inp["rv"]), B.MOM)
    torch.testing.assert_close(f64(rm), rm_ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(f64(rv), rv_ref, rtol=1e-4, atol=1e-5)
    tol, gtol = (2e-2, 5e-2) if bf else (2e-5, 1e-4)
    for res in (True, False):  # the mask bytes of the forward's apply pass / the mask recomputed from x
        r = inp["r"] if res else None
        y, mask = native.bn_fwd_apply(inp["x"], stats, r, True, True)
        assert (mask is not None) == res
        Y = c.rows(y)
        _, y_full = R.bn_apply_ref(X, scale, shift, c.rows(r) if res else None, True)
        torch.testing.assert_close(Y, y_full, rtol=tol, atol=tol)
        pos = Y > 0
        G = ((c.rows32(inp["dy"]) + c.rows32(inp["dy2"])) * pos).to(dtype).double()
        total = torch.zeros(2, C, dtype=torch.float64, device=dev)
        gs = []
        for a, e in bounds:
            if e == a:
                continue
            mk = mask[a * C // V:e * C // V] if res else None
            g, dw, db, sums = native.bn_sync_bwd_reduce(inp["dy"][a:e], inp["x"][a:e], inp["w"], stats, True, True,
                                                        tk, None, None, inp["dy2"][a:e], mk)
            assert not tk.any()
            assert torch.equal(c.rows(g), G[a:e]), f"{tag}: g is not mask * (dy + dy2) rounded once"
            sg, sgx = G[a:e].sum(0), (G[a:e] * (X[a:e] - mean_k)).sum(0)
            G32 = G[a:e].float()
            B._measured(f64(sums[0]), G32.sum(0), sg, f"{tag} sum g", c.loud("sg"))
            B._measured(f64(sums[1]), (G32 * (X32[a:e] - mean_k.float())).sum(0), sgx, f"{tag} sum g (x - mean)",
                        c.loud("sgx"))
            assert torch.equal(db, sums[0].float())
            B._within(f64(dw), f64(sums[1]) * invstd_k, B.ulp32(f64(sums[1]) * invstd_k), f"{tag} local dweight")
            total += sums
            gs.append(g)
        coef = native.bn_sync_coef(total, count, inp["w"], stats)
        T = f64(total)
        A, Bc, Cc = R.sync_coef_ref(T[0], T[1], mean_k, invstd_k, c.w, M)
        A_k, B_k, C_k = f64(coef)
        kk = c.w * invstd_k
        B._within(A_k, A, 4 * B.ulp32(A), f"{tag} coef A")
        B._within(B_k, Bc, 4 * B.ulp32(Bc), f"{tag} coef B")
        B._within(C_k, Cc, 4 * B.ulp32((Bc * mean_k).abs() + (kk * T[0] / M).abs()), f"{tag} coef C")
        dx = torch.cat([native.bn_bwd_apply_g(g, inp["x"][a:e], coef)
                        for g, (a, e) in zip(gs, [b for b in bounds if b[1] > b[0]])])
        DX = c.rows(dx)
        dx_ref = A_k * G + B_k * X + C_k
        bound = 2.0 ** -22 * ((A_k * G).abs() + (B_k * X).abs() + C_k.abs())
        if bf:
            bound = bound + 0.5 * B.bf16_ulp_of(dx_ref)
        B._within(DX, dx_ref, bound, f"{tag} dx from the kernel's coefficients")
        g64 = (c.rows(inp["dy"]) + c.rows(inp["dy2"])) * pos
        dx_full = R.bn_backward_ref(g64, X, mean, invstd, c.w, M)[5]
        torch.testing.assert_close(DX, dx_full, rtol=gtol, atol=gtol)


# ----------------------------------------------------------------------------- stability
@pytest.mark.gpu
@pytest.mark.parametrize("M,row", [(4096, 0), (4096, 2048), (4096, 4095), (262144, 0)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_bn_variance_is_stable_when_the_pivot_row_is_an_outlier(native, dev, dtype, M, row):
    """One row of every channel sits 100 std away (row 0, where the pivot of the shifted sums was
    once taken; the middle and the last row as well): the variance still meets the measured rule."""
    C = 64
    g = torch.Generator(device=dev).manual_seed(M + row)
    x = torch.randn(M, C, device=dev, generator=g)
    x[row] = 100.0
    x = x.to(dtype)
    tk = torch.zeros(B.num_tickets(C, dtype), dtype=torch.int32, device=dev)
    rm1, rv1 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    native.bn_fwd_train(x, None, None, rm1, rv1, nbt, None, False, 1.0, B.EPS, tk, False, True)  # momentum 1
    var_k = rv1.double() * (M - 1) / M
    ref = x.double().var(0, unbiased=False).cpu()
    t32 = x.float().var(0, unbiased=False)
    assert_by_measured_error(var_k, t32, ref, floor=2.0 ** -23 * float(ref.max()),
                             what=f"variance, outlier in row {row} of {M} ({'f32' if dtype == F32 else 'bf16'})")


# ----------------------------------------------------------------------------- knobs (child processes)
_KNOB_PROBE = r"""
import sys, torch
from pytorch_distributed_training_tutorials_amd import native
from tests import _bn_raw as B
nat, dev, tc, out = native(), torch.device("cuda", 0), int(sys.argv[2]), {}
for dt, M, C in B.KNOB_SHAPES:
    inp = B.make_inputs(M, C, getattr(torch, dt), B.KNOB_SEED, dev)
    for i, v in enumerate(B.KNOB_VARIANTS):
        out[f"{dt}-{M}x{C}/{i}"] = B.to_cpu(B.run_raw(nat, inp, v, tc))
torch.cuda.synchronize()
torch.save(out, sys.argv[1])
"""

KNOBS = [dict(PTDT_BN_TC="4"), dict(PTDT_BN_TC="16"), dict(PTDT_BN_TC="64"), dict(PTDT_BN_AU="2"),
         dict(PTDT_BN_AU="4", PTDT_BN_APPLY_BLOCKS="1"), dict(PTDT_BN_DIR="15"),
         dict(PTDT_BN_INTERLEAVE="0", PTDT_BN_RPT="1", PTDT_BN_RED_BLOCKS="64")]
_ALL_KNOBS = ("PTDT_BN_TC", "PTDT_BN_AU", "PTDT_BN_APPLY_BLOCKS", "PTDT_BN_DIR", "PTDT_BN_INTERLEAVE", "PTDT_BN_RPT",
              "PTDT_BN_RED_BLOCKS", "PTDT_BN_FENCE")


def _child(probe, args, knobs):
    env = {k: v for k, v in os.environ.items() if k not in _ALL_KNOBS}
    env.update(knobs, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, "-c", probe, *args], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "+".join(f"{a[8:]}={b}" for a, b in k.items()))
def test_bn_knob_variants_meet_the_same_bounds(tmp_path, knobs):
    """The knobs are read once per process: one fresh child per setting runs forward + backward
    through the raw bindings and saves every output; the same layered assertions apply (a child's
    sums may differ from the default process in the last bits, the bounds do not move)."""
    path = str(tmp_path / "out.pt")
    _child(_KNOB_PROBE, [path, knobs.get("PTDT_BN_TC", "0")], knobs)
    out = torch.load(path, weights_only=True)
    for dt, M, C in B.KNOB_SHAPES:
        inp = B.make_inputs(M, C, getattr(torch, dt), B.KNOB_SEED, "cpu")
        case = B.Case(inp, "cpu")
        for i, v in enumerate(B.KNOB_VARIANTS):
            B.check_raw(case, v, out[f"{dt}-{M}x{C}/{i}"], f"{knobs} {dt}-{M}x{C} {tuple(int(f) for f in v)}")


_TC4_MODULE_PROBE = r"""
import sys, torch
from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d, batch_norm_act
from tests import _bn_raw as B
dev = torch.device("cuda", 0)
inp = B.make_inputs(4099, 80, torch.float32, B.KNOB_SEED, dev)
bn = BatchNorm2d(80).to(dev)
with torch.no_grad():
    bn.weight.copy_(inp["w"]); bn.bias.copy_(inp["b"])
try:
    out = {"y": batch_norm_act(inp["x"], bn, relu=True).detach().cpu(), "tickets": bn._bn_tickets.cpu()}
except RuntimeError as e:
    out = {"error": str(e)}
torch.save(out, sys.argv[1])
"""


@pytest.mark.gpu
def test_bn_module_under_a_narrow_forced_tile_is_right_or_refused(tmp_path):
    """PTDT_BN_TC=4 halves the fp32 tile: 80 channels are 5 tiles, and the module's ticket buffer
    (one per 32 channels) has 3. Either the result is right or the binding says "tickets"."""
    path = str(tmp_path / "out.pt")
    _child(_TC4_MODULE_PROBE, [path], dict(PTDT_BN_TC="4"))
    out = torch.load(path, weights_only=True)
    if "error" in out:
        assert "tickets" in out["error"], out["error"]
        return
    inp = B.make_inputs(4099, 80, F32, B.KNOB_SEED, "cpu")
    _, _, _, scale, shift = R.bn_stats_ref(inp["x"], inp["w"], inp["b"], B.EPS32)
    _, y_ref = R.bn_apply_ref(inp["x"], scale, shift, None, True)
    torch.testing.assert_close(out["y"].double(), y_ref, rtol=2e-5, atol=2e-5)
    assert not out["tickets"].any()


# ----------------------------------------------------------------------------- wide channel counts
WIDE = [(BF16, 3280), (BF16, 5464), (BF16, 8192), (BF16, 8200), (F32, 3280), (F32, 5464), (F32, 8192)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,C", WIDE, ids=lambda p: str(p).replace("torch.", ""))
@pytest.mark.parametrize("res", [False, True], ids=["relu", "relu_res"])
def test_bn_wide_channel_counts(native, dev, dtype, C, res):
    """Just over the channel counts at which the 5 C, 3 C and 2 C floats of the elementwise passes'
    LDS tables cross 64 KiB (opt-in needed), and over what 160 KiB can hold (8192 channels: the
    composite path takes over, the binding refuses); 8192 itself, the widest the native path takes, fills
    the 160 KiB exactly in the backward without a residual. Through batch_norm_act, at the end-to-end
    tolerances of test_native_bn_train_fwd_bwd."""
    from pytorch_distributed_training_tutorials_amd.ops import norm

    assert native.bn_max_channels() == 8192
    M = 64
    inp = B.make_inputs(M, C, dtype, C, dev)
    bn = norm.BatchNorm2d(C).to(dev)
    with torch.no_grad():
        bn.weight.copy_(inp["w"])
        bn.bias.copy_(inp["b"])
        bn.running_mean.copy_(inp["rm"])
        bn.running_var.copy_(inp["rv"])
    x = inp["x"].clone().requires_grad_()
    r = inp["r"].clone().requires_grad_() if res else None
    y = norm.batch_norm_act(x, bn, residual=r, relu=True)
    is_native = type(y.grad_fn).__name__.startswith("_BatchNormActFn")
    assert is_native == (C <= native.bn_max_channels()), "a supported width must run on the native kernels"
    y.backward(inp["dy"])
    torch.cuda.synchronize()
    if not is_native:
        with pytest.raises(RuntimeError, match="at most 8192 channels"):
            native.bn_fwd_train(inp["x"], None, None, None, None, None, None, True, 0.1, 1e-5, None, False, False)
        with pytest.raises(RuntimeError, match="at most 8192 channels"):
            native.bn_apply(inp["x"], None, inp["w"], inp["b"], True)
    c = B.Case(inp, "cpu")
    bf = dtype == BF16
    tol, gtol, wtol = (2e-2, 5e-2, 1e-3 * M ** 0.5) if bf else (2e-5, 1e-4, 1e-3)
    mean, var, invstd, scale, shift = c.stats[True]
    Y = c.rows(y)
    _, y_full = R.bn_apply_ref(c.X, scale, shift, c.rows(inp["r"]) if res else None, True)
    torch.testing.assert_close(Y, y_full, rtol=tol, atol=tol)
    g64 = c.rows(inp["dy"]) * (Y > 0)
    db, dw, _, _, _, dx = R.bn_backward_ref(g64, c.X, mean, invstd, c.w, M)
    torch.testing.assert_close(c.rows(x.grad), dx, rtol=gtol, atol=gtol)
    if res:
        torch.testing.assert_close(c.rows(r.grad), g64, rtol=gtol, atol=gtol)
    torch.testing.assert_close(c.f64(bn.weight.grad), dw, rtol=1e-3, atol=wtol)
    torch.testing.assert_close(c.f64(bn.bias.grad), db, rtol=1e-3, atol=wtol)
    rm_ref, rv_ref = R.bn_running_ref(mean, var, M, c.f64(inp["rm"]), c.f64(inp["rv"]), bn.momentum)
    torch.testing.assert_close(c.f64(bn.running_mean), rm_ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(c.f64(bn.running_var), rv_ref, rtol=1e-4, atol=1e-5)
    assert int(bn.num_batches_tracked) == 1
