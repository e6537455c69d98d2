"""The layer-wise optimizers' definition in plain torch: lists of tensors in, lists out, float64
unless another ``dtype`` is asked for (the tolerance check evaluates the same formulae in float32).

With ``g' = gscale * gcoef * g`` (``gscale`` = -1 under ``maximize``, ``gcoef`` the clip coefficient):

LARS    w = ||p||, n = ||g'||
        ratio = trust_coefficient * w / (n + weight_decay * w + eps)  if w > 0 and n > 0 else 1
        d = ratio * (g' + weight_decay * p), then torch.optim.SGD's momentum step on d

LAMB    m = b1 m + (1 - b1) g', v = b2 v + (1 - b2) g'^2
        u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + weight_decay * p
        w = ||p||, n = ||u||, ratio = w / n  if adapt and w > 0 and n > 0 else 1
        p -= lr * ratio * u
"""
from __future__ import annotations

import torch


def _as(t, dtype):
    return t.detach().to("cpu", dtype)


def _ratio_or_one(ok, value, dtype):
    return value if ok else torch.ones((), dtype=dtype)


def lars_step(ps, gs, bufs, *, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
              maximize=False, trust_coefficient=1e-3, eps=1e-8, gcoef=1.0, dtype=torch.float64):
    """One step. ``bufs[i]`` is None before parameter i's first update. Returns
    ``(new_ps, new_bufs, ratios)``; a parameter whose gradient is None passes through."""
    out_p, out_b, ratios = [], [], []
    for p, g, buf in zip(ps, gs, bufs):
        if g is None:
            out_p.append(p), out_b.append(buf), ratios.append(None)
            continue
        p, g = _as(p, dtype), _as(g, dtype) * (-1.0 if maximize else 1.0) * gcoef
        w, n = torch.linalg.vector_norm(p), torch.linalg.vector_norm(g)
        ratio = torch.ones((), dtype=dtype)
        if trust_coefficient != 0:
            ratio = _ratio_or_one(bool(w > 0) and bool(n > 0), trust_coefficient * w / (n + weight_decay * w + eps),
                                  dtype)
        d = ratio * (g + weight_decay * p)
        if momentum != 0:
            buf = d.clone() if buf is None else momentum * _as(buf, dtype) + (1 - dampening) * d
            d = d + momentum * buf if nesterov else buf
        out_p.append(p - lr * d), out_b.append(buf), ratios.append(float(ratio))
    return out_p, out_b, ratios


def lamb_step(ps, gs, ms, vs, t, *, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, bias_correction=True,
              adapt=True, maximize=False, gcoef=1.0, dtype=torch.float64):
    """One step, ``t`` the 1-based count of this update. ``ms[i]`` / ``vs[i]`` None mean zeros.
    Returns ``(new_ps, new_ms, new_vs, ratios)``."""
    b1, b2 = betas
    bc1 = 1 - b1 ** t if bias_correction else 1.0
    bc2 = 1 - b2 ** t if bias_correction else 1.0
    out_p, out_m, out_v, ratios = [], [], [], []
    for p, g, m, v in zip(ps, gs, ms, vs):
        if g is None:
            out_p.append(p), out_m.append(m), out_v.append(v), ratios.append(None)
            continue
        p, g = _as(p, dtype), _as(g, dtype) * (-1.0 if maximize else 1.0) * gcoef
        m = (1 - b1) * g if m is None else b1 * _as(m, dtype) + (1 - b1) * g
        v = (1 - b2) * g * g if v is None else b2 * _as(v, dtype) + (1 - b2) * g * g
        u = (m / bc1) / (v.sqrt() / bc2 ** 0.5 + eps) + weight_decay * p
        w, n = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
        ratio = _ratio_or_one(adapt and bool(w > 0) and bool(n > 0), w / n, dtype)
        out_p.append(p - lr * ratio * u), out_m.append(m), out_v.append(v), ratios.append(float(ratio))
    return out_p, out_m, out_v, ratios


def lars_run(ps, grads, steps_kw, **kw):
    """``len(grads)`` steps from fresh state; ``grads[k]`` the gradient list of step k, ``steps_kw[k]``
    what changes per step (e.g. ``lr``, ``gcoef``). Returns (parameters, buffers, last ratios)."""
    bufs, ratios = [None] * len(ps), None
    for gs, extra in zip(grads, steps_kw):
        ps, bufs, ratios = lars_step(ps, gs, bufs, **{**kw, **extra})
    return ps, bufs, ratios


def lamb_run(ps, grads, steps_kw, **kw):
    ms, vs, ratios = [None] * len(ps), [None] * len(ps), None
    for t, (gs, extra) in enumerate(zip(grads, steps_kw), start=1):
        ps, ms, vs, ratios = lamb_step(ps, gs, ms, vs, t, **{**kw, **extra})
    return ps, ms, vs, ratios
