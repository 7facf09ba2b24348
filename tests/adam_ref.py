"""Adam / AdamW's definition in numpy: what yv3_adam_step (csrc/optim.hip) must compute, bit for bit (include/yv3.h states the same).

It is torch 2.10's ``_single_tensor_adam`` on its non-capturable, non-differentiable path with every operation rounded once to
fp32 (``.astype(np.float32)`` after each, no fused multiply-add) and every scalar that enters a tensor operation rounded to fp32
first, as torch's GPU kernels take it.  ``step`` is the parameter's step count after the increment; scalars marked (double) are
Python floats.  On a parameter's first step ``m``, ``v`` and ``vmax`` are None and taken as +0.  Denormals are kept; NaN and inf
follow from the operations.  Not a test module: test_adam_host.py and test_gpu_adam.py import it; the clip coefficient, the norm
and ``same_bits`` are those of tests/optim_ref.py.

The bar (``K``).  After one step from shared fp32 state the fp32 result is held to the float64 step ``adam64`` by
``|x' - x64| <= K * 2^-24 * Mx`` for x in (m, v, p), every element counted.  K is the number of fp32 roundings on the longest path
of the definition, from ``g`` to ``p'`` under L2 decay with a clip coefficient:

    g * coef                                   1
    f32(weight_decay), its product with p,
    the sum with g                             3      -> 4 roundings in g, which enter v twice (g * g)           8
    f32(1 - beta2), its product with g,
    the product with g, the sum with v         4                                                                 12
    sqrt                                       1                                                                 13
    f32(bc2 ** 0.5), the quotient              2                                                                 15
    f32(eps), the sum                          2                                                                 17
    m / den                                    1                                                                 18
    f32(-(lr / bc1)), its product              2                                                                 20
    p + ...                                    1                                                                 21

Each is at most half an ulp relative to a magnitude the scales below bound.  The paths to m' (f32(1 - beta1), d, 1 - w, the
product, the difference: 5 after g's 4) and to v' (12 and the two of f32(beta2) * v) are shorter.

Where a result is subnormal (g * g is for |g| < 1e-19) a rounding errs by up to half the smallest subnormal, 2^-150, whatever its
size, which no relative bound covers; the bar is therefore ``K * 2^-24 * Mx + K_TINY * 2^-150``.  ``K_TINY = 3`` counts the roundings
whose subnormal result reaches x' at unit gain -- sums and differences of subnormals are exact, so only products count: into m',
g * coef, f32(weight_decay) * p and w * d (or d * (1 - w)); into v', v * f32(beta2) and (f32(1 - beta2) * g) * g (the inner
product's absolute error is multiplied by |g| < 1); into p', p * decay and f32(-(lr / bc1)) * (m / den) -- a subnormal m' carries its
2^-150 into p' times (lr / bc1) / den, which is far below 2^-24 |p| for any p that is not itself near the subnormals.  The term is
at most a seventh of the first wherever Mx is a normal fp32.
"""
import numpy as np

from tests.optim_ref import same_bits                               # noqa: F401  (two NaNs compare equal)

F32 = np.float32
U24 = 2.0 ** -24          # half an fp32 ulp, relative
TINY = 2.0 ** -150        # half the smallest fp32 subnormal: a rounding's error where the result is subnormal
K = 21.0
K_TINY = 3.0


def f32(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, dtype=np.float64).astype(F32)


def maximum(a, b):
    """torch.maximum: a NaN on either side is kept; otherwise the larger, b on a tie."""
    with np.errstate(all="ignore"):
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(a > b, a, b))).astype(F32)


def scalars(step, lr, betas, eps, weight_decay, decoupled):
    """The fp32 scalars of one step, reduced in double first: (w, beta2, 1 - beta2, sqrt(bc2), eps, -(lr / bc1), decay).
    decay is f32(1 - lr * weight_decay) when decoupled, f32(weight_decay) otherwise."""
    beta1, beta2 = float(betas[0]), float(betas[1])
    step, lr = float(step), float(lr)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    decay = (1 - lr * weight_decay) if decoupled else weight_decay
    return (F32(1 - beta1), F32(beta2), F32(1 - beta2), F32(bc2 ** 0.5), F32(eps), F32(-(lr / bc1)), F32(decay))


def adam(p, g, m, v, vmax, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False,
         decoupled=False, coef=None):
    """One step of one parameter: returns (p', m', v', vmax'), vmax' None without amsgrad.  m, v, vmax None = the first step."""
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    zero = np.zeros_like(p)
    m = zero if m is None else np.asarray(m, dtype=F32)
    v = zero if v is None else np.asarray(v, dtype=F32)
    vmax = zero if vmax is None else np.asarray(vmax, dtype=F32)
    w, b2, omb2, sbc2, e, nslr, decay = scalars(step, lr, betas, eps, weight_decay, decoupled)
    with np.errstate(all="ignore"):
        if coef is not None:
            g = (g * F32(coef)).astype(F32)
        if maximize:
            g = (-g).astype(F32)
        if decoupled:
            if weight_decay != 0:
                p = (p * decay).astype(F32)
        elif decay != 0:                                            # decided on the fp32 scalar, the one the tensor operation sees
            g = (g + (decay * p).astype(F32)).astype(F32)
        d = (g - m).astype(F32)
        if abs(w) < 0.5:
            m = (m + (w * d).astype(F32)).astype(F32)
        else:
            m = (g - (d * F32(F32(1) - w)).astype(F32)).astype(F32)
        v = (v * b2).astype(F32)
        v = (v + ((omb2 * g).astype(F32) * g).astype(F32)).astype(F32)
        s = v
        if amsgrad:
            s = vmax = maximum(vmax, v)
        den = ((np.sqrt(s).astype(F32) / sbc2).astype(F32) + e).astype(F32)
        p = (p + (nslr * (m / den).astype(F32)).astype(F32)).astype(F32)
    return p, m, v, (vmax if amsgrad else None)


# ---------------------------------------------------------------- float64: what the fp32 definition is held to
def adam64(p, g, m, v, vmax, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False,
           decoupled=False, coef=1.0):
    """The same step in float64 with the hyper-parameters as given (doubles): (p', m', v', vmax', (Mm, Mv, Mp)), the scales
    Mg = |g coef| + (L2 ? wd |p| : 0), Mm = Mg + |m|, Mv = beta2 v + (1 - beta2) Mg^2, Mp = |p| + (lr / bc1) Mm / den."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    zero = np.zeros_like(p)
    m = zero if m is None else np.asarray(m, dtype=np.float64)
    v = zero if v is None else np.asarray(v, dtype=np.float64)
    vmax = zero if vmax is None else np.asarray(vmax, dtype=np.float64)
    beta1, beta2 = float(betas[0]), float(betas[1])
    l2 = weight_decay != 0 and not decoupled
    with np.errstate(all="ignore"):
        g = g * float(coef)
        Mg = np.abs(g) + (weight_decay * np.abs(p) if l2 else 0.0)
        Mm = Mg + np.abs(m)
        Mv = beta2 * v + (1 - beta2) * Mg * Mg
        p0 = np.abs(p)
        if maximize:
            g = -g
        if weight_decay != 0:
            if decoupled:
                p = p * (1 - lr * weight_decay)
            else:
                g = g + weight_decay * p
        m = m + (1 - beta1) * (g - m)
        v = beta2 * v + (1 - beta2) * g * g
        s = v
        if amsgrad:
            s = vmax = np.maximum(vmax, v)
        bc1, bc2 = 1 - beta1 ** float(step), 1 - beta2 ** float(step)
        den = np.sqrt(s) / bc2 ** 0.5 + eps
        p = p - (lr / bc1) * (m / den)
        Mp = p0 + (lr / bc1) * Mm / den
    return p, m, v, (vmax if amsgrad else None), (Mm, Mv, Mp)


def bar_ratios(new, new64, scales):
    """(max |p' - p64| / (U24 Mp + K_TINY / K TINY), the same for m, the same for v), over every element: each must stay <= K.
    new = (p', m', v'), new64 likewise, scales = (Mm, Mv, Mp) of adam64."""
    out = []
    for x, x64, M in ((new[0], new64[0], scales[2]), (new[1], new64[1], scales[0]), (new[2], new64[2], scales[1])):
        x, x64, M = np.asarray(x, dtype=np.float64), np.asarray(x64, dtype=np.float64), np.asarray(M, dtype=np.float64)
        with np.errstate(all="ignore"):
            err = np.abs(x - x64)
            r = np.where(err == 0, 0.0, err / (U24 * M + K_TINY / K * TINY))
        out.append(float(np.max(r)))
    return tuple(out)


# ---------------------------------------------------------------- what both test modules draw and run
SETTINGS = {
    "default": dict(),
    "l2": dict(weight_decay=5e-4),
    "decoupled": dict(weight_decay=1e-2, decoupled=True),
    "amsgrad": dict(amsgrad=True, weight_decay=5e-4),
    "maximize": dict(maximize=True, lr=3e-3),
    "beta1_0": dict(betas=(0.0, 0.999)),
    "beta1_04": dict(betas=(0.4, 0.99), amsgrad=True),          # w = 0.6: lerp's other branch
}


def wide_draws(n, seed):
    """n fp32 gradients, |g| log-uniform in 1e-22 .. 1e2 with random signs and every 17th exactly zero: g * g runs from the
    subnormals (and 0) to 1e4."""
    rng = np.random.default_rng(seed)
    g = (10.0 ** rng.uniform(-22, 2, n) * rng.choice([-1.0, 1.0], n)).astype(F32)
    g[::17] = 0
    return g
