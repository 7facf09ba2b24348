"""The update step's definition in numpy: what csrc/optim.hip must compute, bit for bit (include/yv3.h states the same).

fp32 arrays, ``.astype(np.float32)`` after every operation (one rounding each, no fused multiply-add), and a float64 sum of
squares in the kernels' fixed order: per chunk of CHUNK elements, thread t of THREADS adds the squares of its 4-element groups
t, t + THREADS, ... in element order, a pairwise tree (s[t] += s[t + stride], stride = THREADS/2 .. 1) adds the threads, and the
chunks' partials are added in index order, tensor by tensor.  Not a test module: test_optim_host.py and test_gpu_optim.py import it.
"""
import numpy as np

CHUNK = 16384
THREADS = 256
F32 = np.float32


def chunk_partials(g):
    """float64 partial sums of g^2, one per CHUNK elements of the flattened fp32 array g (the last chunk may be short)."""
    g = np.asarray(g, dtype=F32).reshape(-1)
    n_chunks = -(-g.size // CHUNK)
    sq = np.zeros(n_chunks * CHUNK, dtype=np.float64)
    sq[:g.size] = g.astype(np.float64)
    with np.errstate(all="ignore"):
        sq *= sq                                                   # an fp32 square is exact in float64; the padding adds +0.0
        # [chunk][group round j][thread][element c] -> [j][c][chunk][thread]: thread t adds its 4 * rounds squares in (j, c) order
        sq = np.ascontiguousarray(sq.reshape(n_chunks, CHUNK // (THREADS * 4), THREADS, 4).transpose(1, 3, 0, 2))
        acc = np.zeros((n_chunks, THREADS), dtype=np.float64)
        for j in range(sq.shape[0]):
            for c in range(4):
                acc = acc + sq[j, c]
        stride = THREADS // 2
        while stride:
            acc = acc[:, :stride] + acc[:, stride:2 * stride]
            stride //= 2
    return acc[:, 0]


def sum_of_squares(grads):
    """The float64 sum over all of `grads` (a list of fp32 arrays) in the kernels' order; 0.0 for an empty list."""
    parts = [chunk_partials(g) for g in grads if np.asarray(g).size]
    if not parts:
        return np.float64(0.0)
    with np.errstate(all="ignore"):
        return np.add.accumulate(np.concatenate([np.zeros(1)] + parts))[-1]     # (accumulate adds strictly left to right)


def norm_and_coef(grads, max_norm):
    """(total_norm, coef), both fp32: fp32(sqrt(sum)), min(fp32(max_norm) / (total_norm + 1e-6f), 1) with a NaN kept."""
    with np.errstate(all="ignore"):
        total_norm = F32(np.sqrt(sum_of_squares(grads)))
        denom = F32(total_norm + F32(1e-6))
        q = F32(F32(max_norm) / denom)
        return total_norm, F32(np.minimum(q, F32(1.0)))


def scale(g, coef):
    with np.errstate(all="ignore"):
        return (np.asarray(g, dtype=F32) * F32(coef)).astype(F32)


def sgd(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, coef=None):
    """One step of one parameter: returns (p', buf').  buf None = the parameter's first step (buf' is None when momentum == 0)."""
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    with np.errstate(all="ignore"):
        gs = (g * F32(coef)).astype(F32) if coef is not None else g
        if maximize:
            gs = (-gs).astype(F32)
        d = gs
        if weight_decay != 0:
            wp = (F32(weight_decay) * p).astype(F32)
            d = (gs + wp).astype(F32)
        if momentum != 0:
            if buf is None:
                buf = d.copy()
            else:
                mb = (F32(momentum) * np.asarray(buf, dtype=F32)).astype(F32)
                dd = (F32(1.0 - dampening) * d).astype(F32)          # (1 - dampening) in double, passed as fp32
                buf = (mb + dd).astype(F32)
            if nesterov:
                d = (d + (F32(momentum) * buf).astype(F32)).astype(F32)
            else:
                d = buf
        step = (F32(-lr) * d).astype(F32)
        return (p + step).astype(F32), buf


def same_bits(a, b):
    """a and b hold the same fp32 bits, except that any NaN matches any NaN (payload and sign of a NaN are not part of the definition)."""
    a, b = np.ascontiguousarray(a, dtype=F32).reshape(-1), np.ascontiguousarray(b, dtype=F32).reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---------------------------------------------------------------- float64: what the fp32 definition is held to
def sgd64(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, coef=1.0):
    """The same step in float64 with the hyper-parameters as given (doubles): (p', buf', M), M = |g coef| + wd |p| + momentum |buf|."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    b0 = np.zeros_like(p) if buf is None else np.asarray(buf, dtype=np.float64)
    gs = g * float(coef)
    M = np.abs(gs) + weight_decay * np.abs(p) + momentum * np.abs(b0)
    if maximize:
        gs = -gs
    d = gs + weight_decay * p
    if momentum != 0:
        buf = d.copy() if buf is None else momentum * b0 + (1.0 - dampening) * d
        d = d + momentum * buf if nesterov else buf
    return p - lr * d, buf, M


U24 = 2.0 ** -24          # half an fp32 ulp, relative
BAR = 8.0                 # at most ten half-ulp roundings, each relative to a term of M


def bar_ratios(p0, p1, buf1, p64, buf64, M, lr):
    """max |p' - p'64| / (U24 (|p| + lr M)) and max |buf' - buf'64| / (U24 M): both must stay <= BAR."""
    with np.errstate(all="ignore"):
        rp = np.abs(np.asarray(p1, dtype=np.float64) - p64) / (U24 * (np.abs(np.asarray(p0, dtype=np.float64)) + lr * M) + 1e-300)
        rb = 0.0 if buf64 is None else np.abs(np.asarray(buf1, dtype=np.float64) - buf64) / (U24 * M + 1e-300)
    return float(np.max(rp)), float(np.max(rb))
