"""Affine training augmentation -- rotation, zoom, shear and translation -- for a whole batch on the GPU
(csrc/affine_augment.hip, two launches per batch): the geometric family the reference's README advertises for small custom data
sets (its Data_Augmentation notebook: ``iaa.Sometimes(p, iaa.Affine(...))``), pixels and boxes.

A *program* is one image's transform, a dict::

    {"active": 0 or 1, "shape": (H, W), "fwd": float64[6], "inv": float64[6]}       (+ the drawn values, when sampled)

``fwd`` (2x3, row-major) maps continuous source coordinates to output coordinates and moves the labels; ``inv``, its closed-form
inverse, fetches the pixels; the output has the source's size.  ``fwd = T(C + t) . A . T(-C)`` with C = (W/2, H/2), t = (tx W,
ty H) and ``A = [[s cos th, -s sin(th + ph)], [s sin th, s cos(th + ph)]]`` -- the linear part of skimage's
``AffineTransform(scale, rotation, shear)``, which imgaug's ``Affine`` uses (recalled, not pinned: neither library is a
dependency).  An inactive program (``iaa.Sometimes`` not firing) copies the image and passes its rows through.

``sample_affine`` draws one program per image on the host, ``affine_augment_batch(images, labels, programs)`` runs them and
returns uint8 GPU images and padded float64 GPU labels that ``extra_augment_batch`` and ``augment_batch`` read in place.  The
definitions (Pillow's bilinear ``Image.transform`` for the pixels, pinned by a test; the reference's clip and cut-out rule for the
boxes) are in include/yv3.h and tests/affine_aug_ref.py, DESIGN.md section 8e.2.
"""
import math

import numpy as np
import torch

from . import _ffi
from ._staging import as_images, pad_labels, stage_batch

STREAM = 0x41666669           # "Affi": the second word of the draws' seed, apart from sample_params' and sample_extra's streams

# struct yv3_affine_program (include/yv3.h)
PROGRAM = np.dtype([("active", "<i4"), ("reserved", "<i4"), ("fwd", "<f8", (6,)), ("inv", "<f8", (6,))])


def affine_matrices(H, W, theta=0.0, scale=1.0, shear=0.0, tx=0.0, ty=0.0):
    """``(fwd, inv)`` of an (H, W) image, float64 ``[6]`` each: angles in radians, ``tx`` / ``ty`` fractions of W / H.  ``inv`` is
    the adjugate of ``fwd`` over its determinant."""
    H, W, theta, scale, shear = float(H), float(W), float(theta), float(scale), float(shear)
    a, b = scale * math.cos(theta), -scale * math.sin(theta + shear)
    c, d = scale * math.sin(theta), scale * math.cos(theta + shear)
    cx, cy = W / 2, H / 2
    e = cx + float(tx) * W - (a * cx + b * cy)
    f = cy + float(ty) * H - (c * cx + d * cy)
    det = a * d - b * c
    if det == 0.0 or not math.isfinite(det):
        raise ValueError("the affine map is singular")
    fwd = np.array([a, b, e, c, d, f], dtype=np.float64)
    inv = np.array([d / det, -b / det, (b * f - d * e) / det, -c / det, a / det, (c * e - a * f) / det], dtype=np.float64)
    return fwd, inv


def _range(name, v):
    lo, hi = (float(x) for x in v)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError("%s = (lo, hi) with finite lo <= hi, got %r" % (name, tuple(v)))
    return lo, hi


def sample_affine(seeds, shapes, rotate=(-10, 10), scale=(0.9, 1.1), shear=(-5, 5), translate=(-0.1, 0.1), p=0.5):
    """One program per image, drawn on the host.  ``shapes``: the sources' ``(H, W)``, one per seed.

    ``rotate`` and ``shear`` are ranges in degrees, ``scale`` a range of zoom factors (> 0), ``translate`` a range of shifts as a
    fraction of W (for x) and of H (for y), ``p`` the probability that an image is transformed at all.  For image ``i`` the numpy
    stream ``RandomState([seeds[i], 0x41666669])`` -- a stream of its own: the draws of ``sample_params`` and ``sample_extra`` stay
    where they are -- gives six uniforms, always all six and in this order: ``u = random_sample()``, then ``uniform`` over
    ``rotate``, ``scale``, ``shear``, ``translate`` (x), ``translate`` (y); ``active = u < p``."""
    seeds = [int(s) for s in seeds]
    if shapes is None or len(shapes) != len(seeds):
        raise ValueError("one shape per seed")
    rotate, scale, shear, translate = _range("rotate", rotate), _range("scale", scale), _range("shear", shear), _range("translate", translate)
    if scale[0] <= 0:
        raise ValueError("scale must be > 0, got %r" % (scale,))
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError("p must be in [0, 1]")
    programs = []
    for seed, shape in zip(seeds, shapes):
        H, W = (int(v) for v in (shape.shape if hasattr(shape, "shape") else shape)[:2])
        rng = np.random.RandomState([seed, STREAM])
        u = float(rng.random_sample())
        theta, s, phi = float(rng.uniform(*rotate)), float(rng.uniform(*scale)), float(rng.uniform(*shear))
        tx, ty = float(rng.uniform(*translate)), float(rng.uniform(*translate))
        fwd, inv = affine_matrices(H, W, math.radians(theta), s, math.radians(phi), tx, ty)
        programs.append({"active": int(u < p), "shape": (H, W), "fwd": fwd, "inv": inv,
                         "rotate": theta, "scale": s, "shear": phi, "tx": tx, "ty": ty})
    return programs


def check_affine_programs(programs, shapes):
    """The per-image checks the kernels make on the device (csrc/affine_augment.hip af_check_program), in the same order, on the
    host: raises ``Yv3Error`` with ``code`` YV3_EINVAL before anything is launched.  One check only the host can make: a program
    was computed for one ``shape`` (its centre and its shifts depend on it) and must meet an image of that shape."""
    def fail(i, why):
        err = _ffi.Yv3Error("affine_augment: image %d: %s" % (i, why))
        err.code = _ffi.EINVAL
        raise err
    if len(programs) != len(shapes):
        raise ValueError("one program per image")
    for i, ((H, W), prog) in enumerate(zip(shapes, programs)):
        if H <= 0 or W <= 0:
            fail(i, "empty source")
        if tuple(int(v) for v in prog["shape"]) != (int(H), int(W)):
            fail(i, "the program was computed for shape %r, the image is %r" % (tuple(prog["shape"]), (H, W)))
        for name in ("fwd", "inv"):
            m = np.asarray(prog[name], dtype=np.float64)
            if m.shape != (6,) or not np.all(np.isfinite(m)):
                fail(i, "%s must be six finite coefficients" % name)
        if prog["active"] not in (0, 1, False, True):
            fail(i, "active must be 0 or 1")


def pack_programs(programs):
    """``yv3_affine_program[B]`` as a numpy record array."""
    out = np.zeros(len(programs), dtype=PROGRAM)
    for rec, prog in zip(out, programs):
        rec["active"], rec["fwd"], rec["inv"] = int(prog["active"]), prog["fwd"], prog["inv"]
    return out


def affine_augment_batch(images, labels, programs):
    """``(images_out, labels_out)``: a list of uint8 ``[H,W,3]`` tensors on the current GPU, contiguous views (each 256-aligned)
    into one new allocation -- so ``extra_augment_batch`` and ``augment_batch`` read them in place (their gather path) -- and the
    labels as a zero-padded ``[B,T,5]`` float64 tensor on the GPU, the form ``augment_batch`` takes: kept rows in place, dropped
    rows zeros.

    ``images``: list of uint8 RGB ``[H,W,3]`` numpy arrays or tensors (CPU or GPU), any sizes.  ``labels``: what ``augment_batch``
    takes (a list of ``[n_i,5]`` arrays, a padded ``[B,T,5]`` tensor on either side, or None).  ``programs``: one per image
    (``sample_affine``), checked here (``check_affine_programs``).  Programs, offsets, shapes, host labels and host images go up in
    one copy; GPU images are copied on the device or, as views into one allocation (``TrainBatches``' arena), read where they are
    (``_staging.stage_batch``).  Two launches, ordered on the current stream; neither the sources nor a label tensor passed in
    is written."""
    imgs, shapes = as_images(images)
    B = len(imgs)
    programs = list(programs)
    check_affine_programs(programs, shapes)
    dev_labels, host_labels, T = pad_labels(labels, B)

    st = stage_batch(imgs, shapes, pack_programs(programs), host_labels)
    lib = _ffi.lib()
    out = torch.empty(st.span, dtype=torch.uint8, device="cuda")
    labels_out = torch.empty((B, T, 5), dtype=torch.float64, device="cuda")
    status = torch.empty((2, B), dtype=torch.int32, device="cuda")
    s = _ffi.stream_ptr()
    _ffi.check(lib.yv3_affine_augment(st.src, st.src_bytes, st.src_offsets, st.hw, st.records, B, out.data_ptr(), st.span,
                                      st.out_offsets, status.data_ptr(), s), "yv3_affine_augment")
    if T:
        lab_ptr = dev_labels.data_ptr() if dev_labels is not None else st.labels
        _ffi.check(lib.yv3_affine_labels(lab_ptr, B, T, st.hw, st.records, labels_out.data_ptr(),
                                         status.data_ptr() + 4 * B, s), "yv3_affine_labels")
    return [out[off:off + H * W * 3].view(H, W, 3) for off, (H, W) in zip(st.offsets, shapes)], labels_out
