"""The reference's ``ExtraAugmentations`` (transforms.py:292-329) for a whole batch on the GPU (csrc/extra_augment.hip, six
launches per batch): one of Gaussian / average / median blur, and sharpen, additive Gaussian noise, add, multiply and contrast
normalisation with probability 0.5 each, in random order, on the raw uint8 source.

A *program* is a list of at most six steps, executed in order, each on the whole output of the one before::

    ("GAUSS", sigma)   ("AVERAGE", k)   ("MEDIAN", k)   ("SHARPEN", alpha, lightness)   ("NOISE", scale, per_channel, key)
    ("ADD", v0, v1, v2)   ("MUL", m0, m1, m2)   ("CONTRAST", a0, a1, a2)

``sample_extra`` draws one per image on the host, ``extra_augment_batch(images, programs)`` runs them and returns uint8 GPU
images that ``augment_batch`` reads in place.  The operations' definitions (what of imgaug 0.2.6, cv2 and scipy each restates,
and what is pinned by a test) are in include/yv3.h and tests/extra_aug_ref.py, DESIGN.md section 8e.1.
"""
import math

import numpy as np
import torch

from . import _ffi
from ._staging import as_images, stage_batch

MAX_STEPS, MAX_RADIUS = 6, 12
OPS = {"GAUSS": 1, "AVERAGE": 2, "MEDIAN": 3, "SHARPEN": 4, "NOISE": 5, "ADD": 6, "MUL": 7, "CONTRAST": 8}
_ARGS = {"GAUSS": 1, "AVERAGE": 1, "MEDIAN": 1, "SHARPEN": 2, "NOISE": 3, "ADD": 3, "MUL": 3, "CONTRAST": 3}
MAX_SIDE = 1 << 28
STREAM = 0x58747261           # "Xtra": the second word of the draws' seed, apart from sample_params' stream

# struct yv3_extra_step / yv3_extra_program (include/yv3.h)
STEP = np.dtype([("op", "<i4"), ("k", "<i4"), ("per_channel", "<i4"), ("reserved", "<i4"), ("v", "<f8", (3,)), ("key", "<u8")])
PROGRAM = np.dtype([("n_steps", "<i4"), ("gauss_radius", "<i4"), ("steps", STEP, (MAX_STEPS,)),
                    ("gauss_w", "<f8", (2 * MAX_RADIUS + 1,))])


def sample_extra(seeds, shapes):
    """One program per image, drawn on the host.  ``shapes`` (one per seed, as for ``sample_params``) only sizes the batch: no
    draw depends on an image's size.

    For image ``i`` the numpy stream ``RandomState([seeds[i], 0x58747261])`` -- not the stream ``sample_params`` reads, whose draws
    stay where they are -- gives, in this order (the order is this project's own; imgaug's RNG cannot be reproduced):

      1. the blur: ``randint(3)`` picks Gaussian / average / median, then its value: ``sigma = uniform(0, 3)``, or
         ``k = randint(2, 8)``, or ``k = 2 * randint(1, 6) + 1`` (odd 3..11);
      2. for sharpen, noise, add, multiply, contrast, in this order: ``random_sample() < 0.5`` decides whether the operation is
         present (the coin is always drawn), and a present one draws at once
           sharpen   ``alpha = uniform(0, 0.5)``, ``lightness = uniform(0.75, 1.5)``
           noise     ``scale = uniform(0, 0.05 * 255)``, ``per_channel = random_sample() < 0.5``, the key's low and high words
                     ``randint(0, 2**32)`` twice
           add       ``per_channel = random_sample() < 0.5``, then three ``randint(-5, 6)`` or one for all channels
           multiply  the same with ``uniform(0.8, 1.2)``
           contrast  the same with ``uniform(0.5, 2.0)``;
      3. ``permutation(n)`` of the n present steps (the blur first, then the others in the order above) sets their order."""
    seeds = [int(s) for s in seeds]
    if shapes is None or len(shapes) != len(seeds):
        raise ValueError("one shape per seed")
    programs = []
    for seed in seeds:
        rng = np.random.RandomState([seed, STREAM])
        kind = int(rng.randint(3))
        if kind == 0:
            steps = [("GAUSS", float(rng.uniform(0, 3.0)))]
        elif kind == 1:
            steps = [("AVERAGE", int(rng.randint(2, 8)))]
        else:
            steps = [("MEDIAN", 2 * int(rng.randint(1, 6)) + 1)]

        def three(draw):
            if rng.random_sample() < 0.5:
                return tuple(draw() for _ in range(3))
            return (draw(),) * 3
        if rng.random_sample() < 0.5:
            alpha = float(rng.uniform(0, 0.5))
            steps.append(("SHARPEN", alpha, float(rng.uniform(0.75, 1.5))))
        if rng.random_sample() < 0.5:
            scale = float(rng.uniform(0, 0.05 * 255))
            per_channel = bool(rng.random_sample() < 0.5)
            lo = int(rng.randint(0, 2 ** 32))
            steps.append(("NOISE", scale, per_channel, lo | int(rng.randint(0, 2 ** 32)) << 32))
        if rng.random_sample() < 0.5:
            steps.append(("ADD",) + three(lambda: int(rng.randint(-5, 6))))
        if rng.random_sample() < 0.5:
            steps.append(("MUL",) + three(lambda: float(rng.uniform(0.8, 1.2))))
        if rng.random_sample() < 0.5:
            steps.append(("CONTRAST",) + three(lambda: float(rng.uniform(0.5, 2.0))))
        programs.append([steps[j] for j in rng.permutation(len(steps))])
    return programs


def gauss_radius(sigma):
    return int(4.0 * float(sigma) + 0.5)


def gauss_weights(sigma):
    """scipy.ndimage's 1-D Gaussian for ``sigma`` at its default truncate = 4: float64 ``[2r + 1]``, normalised."""
    r = gauss_radius(sigma)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return phi / phi.sum()


def check_programs(programs, shapes):
    """The per-image checks the kernels make on the device (csrc/extra_augment.hip ex_check), in the same order, on the host:
    raises ``Yv3Error`` with ``code`` YV3_EINVAL before anything is launched.  One check only the host can make: a program's
    Gaussian steps (those with a radius above 0) must share one sigma, since `pack_programs` writes one weight table."""
    def fail(i, why):
        err = _ffi.Yv3Error("extra_augment: image %d: %s" % (i, why))
        err.code = _ffi.EINVAL
        raise err

    def finite(*vals):
        return all(isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v) for v in vals)
    if len(programs) != len(shapes):
        raise ValueError("one program per image")
    for i, ((H, W), prog) in enumerate(zip(shapes, programs)):
        if H <= 0 or W <= 0 or H > MAX_SIDE or W > MAX_SIDE:
            fail(i, "a side outside 1..2**28")
        if len(prog) > MAX_STEPS:
            fail(i, "more than %d steps" % MAX_STEPS)
        sigma = None
        for step in prog:
            op = step[0] if len(step) else None
            if op not in OPS:
                fail(i, "unknown operation %r" % (op,))
            a = step[1:]
            if len(a) != _ARGS[op]:
                fail(i, "%s takes %d values" % (op, _ARGS[op]))
            if op == "GAUSS":
                if not finite(a[0]) or a[0] < 0 or a[0] > 1e6:
                    fail(i, "sigma must be finite and >= 0")
                r = gauss_radius(a[0])
                if r > MAX_RADIUS:
                    fail(i, "sigma %r needs radius %d > %d" % (a[0], r, MAX_RADIUS))
                if r > 0 and sigma not in (None, float(a[0])):
                    fail(i, "a program holds one weight table: its Gaussian steps must share one sigma")
                if r > 0:
                    sigma = float(a[0])
            elif op == "AVERAGE":
                if not isinstance(a[0], (int, np.integer)) or not 2 <= a[0] <= 7:
                    fail(i, "average k must be an integer in 2..7")
            elif op == "MEDIAN":
                if not isinstance(a[0], (int, np.integer)) or not 3 <= a[0] <= 11 or a[0] % 2 == 0:
                    fail(i, "median k must be odd, in 3..11")
            elif op == "SHARPEN":
                if not finite(*a):
                    fail(i, "non-finite alpha / lightness")
            elif op == "NOISE":
                if not finite(a[0]) or a[0] < 0:
                    fail(i, "scale must be finite and >= 0")
                if a[1] not in (0, 1, False, True):
                    fail(i, "per_channel must be 0 or 1")
                if not isinstance(a[2], (int, np.integer)) or not 0 <= a[2] < 2 ** 64:
                    fail(i, "the key must be an integer in 0..2**64-1")
            elif op == "ADD":
                if not finite(*a) or any(v != round(v) or abs(v) > 255 for v in a):
                    fail(i, "add takes whole numbers in -255..255")
            elif not finite(*a):
                fail(i, "non-finite %s value" % op.lower())


def pack_programs(programs):
    """``yv3_extra_program[B]`` as a numpy record array (with the Gaussian weights of each program's sigma)."""
    out = np.zeros(len(programs), dtype=PROGRAM)
    for rec, prog in zip(out, programs):
        rec["n_steps"] = len(prog)
        for s, step in zip(rec["steps"], prog):
            op, a = step[0], step[1:]
            s["op"] = OPS[op]
            if op in ("AVERAGE", "MEDIAN"):
                s["k"] = a[0]
            elif op == "NOISE":
                s["v"][0], s["per_channel"], s["key"] = a[0], int(a[1]), a[2]
            else:
                s["v"][:len(a)] = a
            if op == "GAUSS" and gauss_radius(a[0]) > 0:
                w = gauss_weights(a[0])
                rec["gauss_radius"] = gauss_radius(a[0])
                rec["gauss_w"][:w.size] = w
    return out


def extra_augment_batch(images, programs):
    """The programs' outputs: a list of uint8 ``[H,W,3]`` tensors on the current GPU, contiguous views (each 256-aligned) into one
    new allocation -- so ``augment_batch`` reads them in place (its gather path).

    ``images``: list of uint8 RGB ``[H,W,3]`` numpy arrays or tensors (CPU or GPU), any sizes; ``programs``: one per image
    (``sample_extra``), checked here (``check_programs``).  Programs, offsets, shapes and host images go up in one copy; GPU
    images are copied on the device or, as views into one allocation (``TrainBatches``' arena), read where they are
    (``_staging.stage_batch``).  Six launches, ordered on the current stream; the sources are not written."""
    imgs, shapes = as_images(images)
    B = len(imgs)
    programs = list(programs)
    check_programs(programs, shapes)

    st = stage_batch(imgs, shapes, pack_programs(programs))
    lib = _ffi.lib()
    out = torch.empty(st.span, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(1, lib.yv3_extra_augment_workspace_bytes(st.span)), dtype=torch.uint8, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    _ffi.check(lib.yv3_extra_augment(st.src, st.src_bytes, st.src_offsets, st.hw, st.records, B, out.data_ptr(), st.span,
                                     st.out_offsets, ws.data_ptr(), ws.numel(), status.data_ptr(), _ffi.stream_ptr()),
               "yv3_extra_augment")
    return [out[off:off + H * W * 3].view(H, W, 3) for off, (H, W) in zip(st.offsets, shapes)]
