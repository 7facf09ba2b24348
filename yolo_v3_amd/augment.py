"""The reference's training augmentation for a whole batch on the GPU (csrc/augment.hip, three launches per batch).

The reference builds each training sample on the host with imgaug 0.2.6 and cv2 (dataset.py:181-204, transforms.py, the
notebook's ``getTransforms(aug=True)`` with darknet's yolov3 settings)::

    Compose([IaaAugmentations([iaa_hsv_aug(0.1, 1.5, 1.5), iaa_random_crop(0.3), iaa.Fliplr(0.5), IaaLetterbox(dim)]),
             ToTensor()])                                   # max_labels=90, max_label_cols=5

Here the random draws are made on the host (``sample_params``: 8 float64 per image) and the pixels and labels are transformed by
HIP kernels: ``augment_batch(images, labels, dim, params) -> (x [B,3,h,w], target [B,90,5])``, both fp32 on the GPU, ``target``
in the form ``net(x, target)`` takes.  ``TrainBatches`` iterates over the reference's list file: ``epoch_schedule`` gives an epoch's
order, seeds and multi-scale dims, files can be decoded ahead on threads, decoded sources can stay resident on the GPU (read in
place by ``yv3_augment_images_from``), and ``state_dict`` / ``load_state_dict`` resume between two batches.

Differences from the reference, all deliberate:
  - crop and flip are drawn from a numpy stream of the image's seed (``sample_params``), not from imgaug's RNG, which cannot be
    reproduced; the three colour draws are the reference's own (``np.random.seed(seed)``, then ``iaa_hsv_aug``'s order);
  - cv2 is not a dependency: the colour conversions and the cubic resize restate OpenCV's 8-bit integer / fixed-point paths,
    parity with a given cv2 build is unpinned (as for ``letterbox_batch``);
  - the flip of a box uses imgaug 0.2.6's keypoint rule ``(width - 1) - x``, recalled from its source and not pinned by a test;
  - one ``dim`` per batch (the reference may mix dims inside a batch; its collate then returns a list).
Kept on purpose, as the reference does them: a hue sum below 0 clips to 0 and one from 180 to 255 wraps inside HSV2RGB; the pad
after the colour step stays 128; a box partly cropped away is clipped only at the canvas; rows beyond 90 are dropped.
"""
import math
import os
import warnings

import numpy as np
import torch

from . import _ffi
from ._staging import as_images, counters, pad_labels, round_up, stage_batch      # counters: read by tools and tests under this name
from .extra_augment import sample_extra, check_programs, extra_augment_batch      # noqa: F401 (part of this module's interface)
from .affine_augment import sample_affine, check_affine_programs, affine_augment_batch      # noqa: F401 (likewise)

MAX_LABELS = 90
N_PARAMS = 8                 # dhue, dsat, dexp, top, right, bottom, left, flip


def _rand_scale(rng, s):
    """reference transforms.py:81-85 (rand_scale) on the stream ``rng``."""
    v = rng.uniform(1, s)
    if rng.random_sample() < 0.5:
        v = 1 / v
    return v


def sample_params(seeds, hue=0.1, saturation=1.5, exposure=1.5, jitter=0.3, flip=0.5, shapes=None):
    """Per-image augmentation parameters ``[B,8]`` float64 on the CPU: dhue, dsat, dexp, top, right, bottom, left, flip.

    For image ``i`` the numpy stream ``RandomState(seeds[i])`` -- the stream ``np.random.seed(seed)`` sets, as dataset.py:181-186
    seeds it -- gives, in this order: ``dhue = uniform(-hue, hue) * 179``, ``dsat = rand_scale(saturation)``, ``dexp =
    rand_scale(exposure)`` (transforms.py:77-104: the reference's own values), then the CropAndPad sides top, right, bottom, left,
    each ``rint(uniform(-jitter, jitter) * n)`` with n = H for top / bottom and W for right / left (positive pads, negative crops;
    ``keep_one_pixel`` gives crops back where they would leave no pixel),
    and ``flip = random_sample() < flip``.  ``shapes``: the sources' ``(H, W)`` (or arrays, whose first two dims are used)."""
    seeds = [int(s) for s in seeds]
    if shapes is None:
        raise ValueError("sample_params needs the sources' shapes (H, W) to size the crop / pad sides")
    shapes = [tuple(int(v) for v in (s.shape if hasattr(s, "shape") else s)[:2]) for s in shapes]
    if len(shapes) != len(seeds):
        raise ValueError("one shape per seed")
    out = np.zeros((len(seeds), N_PARAMS), dtype=np.float64)
    for i, (seed, (H, W)) in enumerate(zip(seeds, shapes)):
        rng = np.random.RandomState(seed)
        out[i, 0] = rng.uniform(-hue, hue) * 179
        out[i, 1] = _rand_scale(rng, saturation)
        out[i, 2] = _rand_scale(rng, exposure)
        for k, n in zip((3, 4, 5, 6), (H, W, H, W)):
            out[i, k] = np.rint(rng.uniform(-jitter, jitter) * n)
        out[i, 3], out[i, 5] = keep_one_pixel(out[i, 3], out[i, 5], H)
        out[i, 6], out[i, 4] = keep_one_pixel(out[i, 6], out[i, 4], W)
        out[i, 7] = 1.0 if rng.random_sample() < flip else 0.0
    return out


def keep_one_pixel(a, b, n):
    """Two opposite sides of an n-pixel dimension, with crops given back one pixel at a time (the larger crop first) until at least
    one pixel remains -- as imgaug's CropAndPad never crops an image to nothing.  Only tiny sources (n <= 3 at jitter 0.3) need it."""
    while n + a + b < 1:
        if a <= b:
            a += 1
        else:
            b += 1
    return a, b


def letterbox_geometry(H1, W1, dim):
    """IaaLetterbox._compute_height_width_pad (transforms.py:196-205) of an (H1, W1) image on a ``dim`` = (w, h) canvas:
    (resize_w, resize_h, x_pad, y_pad)."""
    out_w, out_h = dim
    ratio = min(out_w / W1, out_h / H1)
    rw, rh = int(W1 * ratio), int(H1 * ratio)
    return rw, rh, (out_w - rw) // 2, (out_h - rh) // 2


def check_params(params, shapes, dim):
    """The per-image checks the kernels make on the device (csrc/augment.hip aug_geometry), in the same order, on the host:
    raises ``Yv3Error`` with ``code`` YV3_EINVAL / YV3_ESHAPE before anything is launched."""
    def fail(code, i, why):
        err = _ffi.Yv3Error("augment: image %d: %s" % (i, why))
        err.code = code
        raise err
    p = np.asarray(params, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != N_PARAMS or p.shape[0] != len(shapes):
        raise ValueError("params must be [B,8] (one row per image)")
    for i, ((H, W), r) in enumerate(zip(shapes, p)):
        if H <= 0 or W <= 0:
            fail(_ffi.EINVAL, i, "empty source")
        if not np.all(np.isfinite(r)):
            fail(_ffi.EINVAL, i, "non-finite parameter")
        if r[1] < 0 or r[2] < 0:
            fail(_ffi.EINVAL, i, "negative dsat / dexp")
        if any(r[k] != np.rint(r[k]) or abs(r[k]) > 2 ** 30 for k in (3, 4, 5, 6)):
            fail(_ffi.EINVAL, i, "crop / pad sides must be whole pixel counts")
        if r[7] not in (0.0, 1.0):
            fail(_ffi.EINVAL, i, "flip must be 0 or 1")
        H1, W1 = H + int(r[3]) + int(r[5]), W + int(r[6]) + int(r[4])
        if H1 < 1 or W1 < 1 or H1 > 2 ** 30 or W1 > 2 ** 30:
            fail(_ffi.ESHAPE, i, "the crop leaves a %d x %d image" % (H1, W1))
        rw, rh, _, _ = letterbox_geometry(H1, W1, dim)
        if rw <= 0 or rh <= 0:
            fail(_ffi.ESHAPE, i, "the letterboxed %d x %d image has no pixel on the canvas" % (H1, W1))


def augment_batch(images, labels, dim, params, max_labels=MAX_LABELS):
    """The training transform of a batch: ``(x [B,3,h,w] fp32, target [B,max_labels,5] fp32)``, both on the current GPU.

    ``images``: list of uint8 RGB ``[H,W,3]`` numpy arrays or tensors (CPU or GPU), any sizes.  ``labels``: list of ``[n_i,5]``
    arrays (cls, cx, cy, w, h relative to the source; n_i may be 0), or a zero-padded ``[B,T,5]`` tensor, or None.  ``dim`` =
    (w, h).  ``params``: ``[B,8]`` float64 on the host (``sample_params``), checked here (``check_params``).

    Host inputs (params, shapes, offsets, labels, host images) go up in one copy and GPU images are copied on the device or, as
    views into one allocation, read in place by ``yv3_augment_images_from`` -- the same bits either way (``_staging.stage_batch``).
    Three kernels follow: colour, crop / pad / flip / letterbox / ToTensor, labels.  Everything is ordered on the current
    stream; the host waits only before a pinned buffer is reused (two are kept)."""
    if not torch.cuda.is_available():
        raise _ffi.Yv3Error("no GPU available: this package has no CPU path")
    out_w, out_h = int(dim[0]), int(dim[1])
    if out_w <= 0 or out_h <= 0 or max_labels <= 0:
        raise ValueError("dim and max_labels must be positive")
    imgs, shapes = as_images(images)
    B = len(imgs)
    if isinstance(params, torch.Tensor):
        if params.is_cuda:
            raise _ffi.Yv3Error("params must be on the host (they are checked there before the launch)")
        params = params.numpy()
    params = np.ascontiguousarray(params, dtype=np.float64)
    check_params(params, shapes, (out_w, out_h))
    dev_labels, host_labels, T = pad_labels(labels, B)

    st = stage_batch(imgs, shapes, params, host_labels)
    counters["batches"] += 1
    lib = _ffi.lib()
    x = torch.empty((B, 3, out_h, out_w), dtype=torch.float32, device="cuda")
    target = torch.empty((B, max_labels, 5), dtype=torch.float32, device="cuda")
    ws = torch.empty(max(1, lib.yv3_augment_workspace_bytes(st.span)), dtype=torch.uint8, device="cuda")
    status = torch.empty((2, B), dtype=torch.int32, device="cuda")
    s = _ffi.stream_ptr()
    if st.gather:          # the colour copies take the batch's own bytes of workspace, not the span of the sources' allocation
        _ffi.check(lib.yv3_augment_images_from(st.src, st.src_bytes, st.src_offsets, st.out_offsets, st.span, st.hw, st.records, B,
                                               x.data_ptr(), out_h, out_w, ws.data_ptr(), ws.numel(), status.data_ptr(), s),
                   "yv3_augment_images_from")
    else:
        _ffi.check(lib.yv3_augment_images(st.src, st.src_bytes, st.src_offsets, st.hw, st.records, B,
                                          x.data_ptr(), out_h, out_w, ws.data_ptr(), ws.numel(), status.data_ptr(), s),
                   "yv3_augment_images")
    if dev_labels is not None:
        lab_ptr = dev_labels.data_ptr() if T else None
    else:
        lab_ptr = st.labels if T else None
    _ffi.check(lib.yv3_augment_labels(lab_ptr, B, T, st.hw, st.records, target.data_ptr(), max_labels, out_h, out_w,
                                      status.data_ptr() + 4 * B, s), "yv3_augment_labels")
    return x, target


def label_path(img_path):
    """reference dataset.py:175-179: the label file of an image."""
    return img_path.replace('jpg', 'txt').replace('images', 'labels')


def read_labels(path):
    """``np.loadtxt(path).reshape(-1, 5)`` (dataset.py:199-200); a missing or empty file means no rows."""
    if not os.path.exists(path):
        return np.zeros((0, 5), dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")              # loadtxt warns on an empty file
        return np.loadtxt(path, dtype=np.float64).reshape(-1, 5)


def epoch_schedule(seed, epoch, n, batch_size, shuffle=True, multiscale=None, dim_interval=10):
    """One epoch's random draws ``(order, seeds, dims)`` for ``n`` images -- a pure host function of its arguments.

    From ``RandomState([seed, epoch])``, in this order: the permutation (when ``shuffle``, else ``arange(n)``), one seed per position
    ``randint(0, 2**31 - 1, size=n)`` and, with ``multiscale=(lo, hi)``, ``randint(lo // 32, hi // 32 + 1, size=ceil(n_batches /
    dim_interval)) * 32``: one square dim per run of ``dim_interval`` batches (the reference's _generate_dims_list, dataset.py:79-93,
    draws 320..608 in steps of 32 but counts its interval in samples; here it is counted in batches, so a batch has one dim).  The
    dims are drawn last, so switching them on moves no other draw.  ``dims``: one ``(w, h)`` per batch, or None without multiscale."""
    n, batch_size, dim_interval = int(n), int(batch_size), int(dim_interval)
    if n < 0 or batch_size < 1 or dim_interval < 1:
        raise ValueError("n >= 0, batch_size >= 1 and dim_interval >= 1 are required")
    if multiscale is not None:
        lo, hi = (int(v) for v in multiscale)
        if lo <= 0 or lo % 32 or hi % 32 or lo > hi:
            raise ValueError("multiscale = (lo, hi): positive multiples of 32 with lo <= hi, got %r" % (tuple(multiscale),))
    rng = np.random.RandomState([int(seed), int(epoch)])
    order = rng.permutation(n) if shuffle else np.arange(n)
    seeds = rng.randint(0, 2 ** 31 - 1, size=n)
    dims = None
    if multiscale is not None:
        n_batches = math.ceil(n / batch_size)
        steps = rng.randint(lo // 32, hi // 32 + 1, size=math.ceil(n_batches / dim_interval)) * 32
        dims = [(int(steps[k // dim_interval]),) * 2 for k in range(n_batches)]
    return order, seeds, dims


def arena_admit(sizes, budget, start=0):
    """The arena's admission rule: ``(offsets, end)`` for images of ``sizes`` bytes offered in this order to an arena of ``budget``
    bytes filled up to ``start``.  Each image that still fits goes to the next 256-aligned offset (first come, first kept, nothing
    is ever evicted); ``offsets[i]`` is None for one that does not fit -- a later, smaller one still may."""
    offsets, pos = [], int(start)
    for n in sizes:
        off = round_up(pos)
        if off + int(n) <= budget:
            offsets.append(off)
            pos = off + int(n)
        else:
            offsets.append(None)
    return offsets, pos


MAX_WORKERS = 16


def _load_source(img_path, lab_path):
    from . import evaluate
    return evaluate.read_image_rgb(img_path), read_labels(lab_path)


def _load_bytes(img_path, lab_path, progressive=False):
    """``decode="gpu"``: a worker only reads the file and parses its header (a file the GPU decoder does not take is decoded
    here by `read_image_rgb`, as in ``decode="pil"``; its exception, if any, is raised at its batch)."""
    from . import jpeg
    src = jpeg.Source(img_path, progressive=progressive)
    if src.error is not None:
        raise src.error
    return src, read_labels(lab_path)


class TrainBatches:
    """Training batches ``(x, target)`` from the reference's list file (one image path per line).

    Each epoch (each ``iter()``) takes its draws from ``epoch_schedule(seed, epoch, ...)``: a permutation (when ``shuffle``), one seed
    per image and, with ``multiscale=(lo, hi)``, one square dim per ``dim_interval`` batches (otherwise ``dim`` = (w, h) for all
    batches).  Images are decoded with ``evaluate.read_image_rgb``, labels read from the reference's label path (a missing file:
    no rows), and every batch goes through ``sample_params(seeds, shapes=..., **aug)`` and ``augment_batch``.  The last batch may be
    smaller.

    ``workers`` > 0 (at most 16): the files of the next ``prefetch`` batches are read and decoded on that many threads while the
    caller trains; parameters are still drawn and ``augment_batch`` still called in batch order on the calling thread, so the
    batches are the same bits, and a worker's exception is raised at the batch its image belongs to.  Closing or dropping the
    iterator cancels what is pending and joins the threads.

    ``cache_bytes`` > 0: one device allocation of that size (made at first use) keeps decoded sources, admitted in batch order by
    ``arena_admit`` until it is full; a resident image is never read or decoded again (its label rows stay on the host), and a
    batch of resident images reaches the kernels without any pixel copy.  ``decoded_bytes()`` is the budget that holds the list.

    ``decode="gpu"`` (default ``"pil"``): the same batches, bit for bit, with the JPEGs decoded on the GPU (`yolo_v3_amd.jpeg`):
    the host -- the workers, when there are any -- only reads the files' bytes and parses their headers; batch k+1's decode is
    enqueued on a stream the loader owns before batch k is handed out, and batch k's consumer waits for batch k's own event
    (measured against a step that fills every CU the decode did not overlap with it: DESIGN.md section 8f); with ``cache_bytes``
    the kernels write straight into the arena.  Files the GPU decoder does not take go through `read_image_rgb` as before.  The
    switch is not part of a ``state_dict``'s config: both settings give the same bits.  ``entropy`` (``"serial"`` by default, or
    ``"parallel"``) is passed on to `jpeg.submit`: the decoder's entropy stage, which changes no bit either.  ``progressive=True``
    (with ``decode="gpu"``) is passed on too: progressive files the parser accepts are decoded on the GPU instead of by
    `read_image_rgb` -- the same bits again, so it is no part of a ``state_dict``'s config either.

    ``extra=True``: the reference's ``ExtraAugmentations`` in front of everything else, as ``Compose([ExtraAugmentations(),
    IaaAugmentations([...]), ToTensor()])`` has them: every batch is ``augment_batch(extra_augment_batch(images,
    sample_extra(seeds, shapes)), ...)`` (`yolo_v3_amd.extra_augment`) -- the extras run on the raw source (the arena keeps raw
    sources), labels are untouched.  The switch is part of a ``state_dict``'s config when it is on.

    ``affine`` (None / False, True, or a dict of ``sample_affine``'s keyword arguments; True takes its defaults): rotation, zoom,
    shear and shift (`yolo_v3_amd.affine_augment`) in front of the extras: every batch is ``augment_batch(*affine_augment_batch(
    images, labels, sample_affine(seeds, shapes, **affine)), ...)``, with ``extra_augment_batch`` on the warped images in between
    when ``extra`` is on too -- so blur, sharpen and noise act on the warped image and are not interpolated.  The boxes move with
    the pixels.  The setting is part of a ``state_dict``'s config when it is on.

    ``state_dict()`` / ``load_state_dict()`` resume between two batches with the same data order."""

    def __init__(self, list_file, batch_size, dim, seed, shuffle=True, max_labels=MAX_LABELS, multiscale=None, dim_interval=10,
                 workers=0, prefetch=2, cache_bytes=0, decode="pil", extra=False, entropy="serial", progressive=False,
                 affine=None, **aug):
        if decode not in ("pil", "gpu"):
            raise ValueError("decode must be 'pil' or 'gpu'")
        if entropy not in ("serial", "parallel"):
            raise ValueError("entropy must be 'serial' or 'parallel'")
        self.decode, self._side, self.extra, self.entropy = decode, None, bool(extra), entropy
        self.progressive = bool(progressive)
        if affine is None or affine is False:
            self.affine = None
        else:
            self.affine = {} if affine is True else {k: (float(v) if k == "p" else [float(x) for x in v]) for k, v in dict(affine).items()}
            sample_affine([], [], **self.affine)         # validates the names and the ranges
        with open(list_file, 'r') as f:
            self.img_list = [line.strip() for line in f.readlines() if line.strip()]
        self.label_list = [label_path(p) for p in self.img_list]
        self.batch_size, self.dim, self.seed, self.shuffle = int(batch_size), tuple(dim), int(seed), shuffle
        self.max_labels, self.aug, self.epoch = max_labels, aug, 0
        self.multiscale = None if multiscale is None else tuple(int(v) for v in multiscale)
        self.dim_interval = int(dim_interval)
        self.workers, self.prefetch, self.cache_bytes = min(max(int(workers), 0), MAX_WORKERS), max(int(prefetch), 0), int(cache_bytes)
        epoch_schedule(self.seed, 0, 0, self.batch_size, self.shuffle, self.multiscale, self.dim_interval)    # validates
        self._arena, self._arena_end, self._resident = None, 0, {}     # resident: list index -> (image view in the arena, label rows)
        self._pos, self._resume = None, None

    def __len__(self):
        return math.ceil(len(self.img_list) / self.batch_size)

    def decoded_bytes(self):
        """The ``cache_bytes`` that keeps every image of the list resident: the sum of their 256-aligned ``H * W * 3``, from the
        files' headers (``evaluate.image_size``)."""
        from . import evaluate
        return sum(round_up(w * h * 3) for w, h in (evaluate.image_size(p) for p in self.img_list))

    def resident_images(self):
        """How many images of the list are resident in the arena."""
        return len(self._resident)

    # ---- resume ---------------------------------------------------------------------------------------------------------------
    def _config(self):
        config = {"n": len(self.img_list), "batch_size": self.batch_size, "shuffle": bool(self.shuffle),
                  "multiscale": None if self.multiscale is None else list(self.multiscale), "dim_interval": self.dim_interval,
                  "aug": dict(self.aug)}
        if self.extra:                                   # absent when off: a state written before the switch existed still loads
            config["extra"] = True
        if self.affine is not None:                      # likewise
            config["affine"] = dict(self.affine) or True
        return config

    def state_dict(self):
        """``{"seed", "epoch", "batch", "config"}``: ``epoch`` is the epoch of the iteration in progress and ``batch`` the number of
        batches it has yielded so far.  Every draw derives from ``(seed, epoch)``, so no RNG state is kept.  (The reference's
        DataHelper, dataset.py:361-372, saves ``current_batch`` before incrementing it and resumes at ``+ 1``; ``batch`` here is
        already the index of the next batch.)"""
        epoch, batch = self._resume or self._pos or (self.epoch, 0)
        return {"seed": self.seed, "epoch": epoch, "batch": batch, "config": self._config()}

    def load_state_dict(self, state):
        """The next ``iter()`` continues ``state``'s epoch at its batch, or starts the following epoch if that one was complete.
        The seed is taken from ``state``; a ``config`` that differs from this loader's raises ``ValueError``."""
        if state["config"] != self._config():
            raise ValueError("state_dict of another loader: config %r, this loader's is %r" % (state["config"], self._config()))
        epoch, batch = int(state["epoch"]), int(state["batch"])
        if epoch < 0 or batch < 0 or batch > len(self):
            raise ValueError("state_dict out of range: epoch %d, batch %d of %d" % (epoch, batch, len(self)))
        self.seed, self._pos = int(state["seed"]), None
        if batch < len(self):
            self.epoch, self._resume = epoch, (epoch, batch)
        else:
            self.epoch, self._resume = epoch + 1, None

    # ---- the host half --------------------------------------------------------------------------------------------------------
    def host_batches(self):
        """One epoch's batches as ``(images, labels, params, dim)``, everything ``augment_batch`` takes, without touching a GPU.
        ``images[i]`` is None for a source that is resident in the arena (``params`` were drawn with its recorded shape); with
        ``decode="gpu"`` it is the undecoded `jpeg.Source` (``.shape`` from its header)."""
        for _, images, labels, params, dim, _, _ in self._host_batches():
            yield images, labels, params, dim

    def _host_batches(self):
        if self._resume is not None:
            (epoch, first), self._resume = self._resume, None
        else:
            epoch, first = self.epoch, 0
        self.epoch = epoch + 1
        self._pos = (epoch, first)
        n, bs = len(self.img_list), self.batch_size
        order, seeds, dims = epoch_schedule(self.seed, epoch, n, bs, self.shuffle, self.multiscale, self.dim_interval)
        n_batches = len(self)
        pool, pending = None, {}                         # pending: batch -> one future (or None: resident) per image
        load = _load_source
        if self.decode == "gpu":
            progressive = self.progressive

            def load(img_path, lab_path):
                return _load_bytes(img_path, lab_path, progressive)
        if self.workers > 0:
            from concurrent.futures import ThreadPoolExecutor
            pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="yv3-decode")
        try:
            for k in range(first, n_batches):
                idx = [int(j) for j in order[k * bs:(k + 1) * bs]]
                if pool is not None:
                    for q in range(k, min(k + self.prefetch, n_batches - 1) + 1):
                        if q not in pending:
                            pending[q] = [None if j in self._resident else pool.submit(load, self.img_list[j], self.label_list[j])
                                          for j in (int(j) for j in order[q * bs:(q + 1) * bs])]
                    loaded = [None if f is None else f.result() for f in pending.pop(k)]
                else:
                    loaded = [None if j in self._resident else load(self.img_list[j], self.label_list[j]) for j in idx]
                images, labels, shapes = [], [], []
                for j, got in zip(idx, loaded):
                    if got is None:
                        view, rows = self._resident[j]
                        images.append(None)
                        shapes.append(tuple(view.shape[:2]))
                    else:
                        img, rows = got
                        images.append(img)
                        shapes.append(tuple(img.shape[:2]))
                    labels.append(rows)
                params = sample_params(seeds[k * bs:k * bs + len(idx)], shapes=shapes, **self.aug)
                programs = sample_extra(seeds[k * bs:k * bs + len(idx)], shapes) if self.extra else None
                warps = sample_affine(seeds[k * bs:k * bs + len(idx)], shapes, **self.affine) if self.affine is not None else None
                self._pos = (epoch, k + 1)
                yield idx, images, labels, params, self.dim if dims is None else dims[k], programs, warps
        finally:
            if pool is not None:
                pool.shutdown(wait=True, cancel_futures=True)

    # ---- the device half ------------------------------------------------------------------------------------------------------
    def _admit(self, idx, images, labels):
        """Replace resident sources by their arena views, and admit the decoded ones that still fit (in batch order)."""
        new = [i for i, j in enumerate(idx) if j not in self._resident]
        offsets, _ = arena_admit([images[i].size for i in new], self.cache_bytes, self._arena_end)
        out = list(images)
        for i, off in zip(new, offsets):
            if off is None:
                continue
            if self._arena is None:
                self._arena = torch.empty(self.cache_bytes, dtype=torch.uint8, device="cuda")
            img = images[i]
            view = self._arena[off:off + img.size].view(img.shape)
            view.copy_(torch.from_numpy(img))
            counters["upload_bytes"] += img.size
            self._arena_end = off + img.size
            self._resident[idx[i]] = (view, labels[i])
        for i, j in enumerate(idx):
            if j in self._resident:
                out[i] = self._resident[j][0]
        return out

    # ---- decode="gpu" ---------------------------------------------------------------------------------------------------------
    def _launch(self, batch):
        """Enqueue the decode of a host batch's sources on the loader's stream: those the arena admits (in batch order, by the
        same rule and so at the same offsets as ``decode="pil"``) straight into it, the others into a buffer of the batch."""
        from . import jpeg
        idx, images, labels, params, dim, _, _ = batch
        new = [i for i, im in enumerate(images) if im is not None]
        admitted, offsets = [], []
        if self.cache_bytes > 0 and new:
            offs, _ = arena_admit([images[i].nbytes for i in new], self.cache_bytes, self._arena_end)
            for i, off in zip(new, offs):
                if off is None:
                    continue
                if self._arena is None:
                    self._arena = torch.empty(self.cache_bytes, dtype=torch.uint8, device="cuda")
                    self._side.wait_stream(torch.cuda.current_stream())      # whatever used these bytes before has finished
                admitted.append(i)
                offsets.append(off)
                self._arena_end = off + images[i].nbytes
        rest = [i for i in new if i not in admitted]
        jobs = []
        if admitted:
            jobs.append((admitted, jpeg.submit([images[i] for i in admitted], stream=self._side, dst=(self._arena, offsets),
                                                   entropy=self.entropy, progressive=self.progressive)))
        if rest:
            jobs.append((rest, jpeg.submit([images[i] for i in rest], stream=self._side, entropy=self.entropy,
                                           progressive=self.progressive)))
        return batch, admitted, jobs, self._pos

    def _complete(self, launched):
        batch, admitted, jobs, pos = launched
        idx, images, labels, params, dim, programs, warps = batch
        out = list(images)
        for which, job in jobs:
            for i, view in zip(which, job.finish()):         # raises what read_image_rgb raises for a file nobody can decode
                out[i] = view
        for i in admitted:
            self._resident[idx[i]] = (out[i], labels[i])
        for i, j in enumerate(idx):
            if out[i] is None:
                out[i] = self._resident[j][0]
        self._pos = pos                                      # the host half runs one batch ahead: report the batch handed out
        if warps is not None:
            out, labels = affine_augment_batch(out, labels, warps)
        if programs is not None:
            out = extra_augment_batch(out, programs)
        return augment_batch(out, labels, dim, params, self.max_labels)

    def _iter_gpu(self):
        if self._side is None:
            self._side = torch.cuda.Stream(priority=-1)      # few, long-running workgroups (no measured effect under a CU-filling step)
        host = self._host_batches()
        try:
            ahead = None
            for batch in host:
                launched = self._launch(batch)               # batch k+1 is enqueued before batch k is handed out
                if ahead is not None:
                    x = self._complete(ahead)
                    ahead = launched
                    yield x
                    continue
                ahead = launched
            if ahead is not None:
                yield self._complete(ahead)
        finally:
            host.close()

    def __iter__(self):
        if self.decode == "gpu":
            return self._iter_gpu()
        return self._iter_pil()

    def _iter_pil(self):
        host = self._host_batches()
        try:
            for idx, images, labels, params, dim, programs, warps in host:
                if self.cache_bytes > 0:
                    images = self._admit(idx, images, labels)
                if warps is not None:
                    images, labels = affine_augment_batch(images, labels, warps)
                if programs is not None:
                    images = extra_augment_batch(images, programs)
                yield augment_batch(images, labels, dim, params, self.max_labels)
        finally:
            host.close()                                 # joins the decode threads when the iterator is closed or dropped
