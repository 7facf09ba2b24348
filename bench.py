#!/usr/bin/env python
"""Headline benchmark: YOLOv3 inference hot path on MI355X (BASELINE.json metric: images/sec + ms/img at
416x416 bs=64 on 1/2/4/8 GPUs; NMS boxes delta vs ref).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch 64 | --global-batch G] [--size 416] [--dtype f32] [--full]

A plain run measures the headline alone: it sets up, warms up, times the steps, writes --dump-outputs if given and prints the
result line.  Everything that takes runs of its own -- the one-lane roofline pass, the PMC child passes, the other modes and
configs, the PCIe passes, the CPU baseline and boxes_delta -- and the full-object side file belong to `--full`.

A step = one pass of the whole hot path over one batch of synthetic images already resident in HBM, run through
the PRODUCT entry points: `Detector.run_device` at N = 1 (yolo_v3_amd/detect.py: conv0 -> 74 convs with the YOLO decode
fused into the head convs -> confidence filter -> per-class greedy NMS) and `ShardedDetector.run_device` at N > 1
(yolo_v3_amd/dist.py: the same per-rank pipeline + the ONE all-gather of the [B_local, cap+1, 7] payload -- boxes plus a
row with candidate / kept counts and the kernels' status word -- over RCCL; it is what `detect_sharded` runs), then
the result is copied to pinned host memory asynchronously.  The list conversion (`assemble`, the path's one host sync)
is outside the timed region and runs once after it (it also checks the status word).  `--dump-outputs DIR` then writes what
the last timed step computed (final boxes, counts, a fixed sample of the decoded detections) as .npy files: weights and scenes are
seeded, so two builds run with the same arguments can be compared output for output (`dump_outputs`).

Launch: `python bench.py --gpus N` with N > 1 and no torchrun environment RE-LAUNCHES ITSELF under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` (one rank per GPU) and
fails loudly when fewer than N GPUs are visible (YV3_DIST_BACKEND=gloo: rehearsal mode, ranks may share a GPU and gloo
carries the gather); launched under torchrun it requires WORLD_SIZE == --gpus.  `--dry-run` exercises launcher,
rendezvous, the product's pack -> gather -> assemble composition and the JSON line on CPU tensors (no GPU, no kernels;
tests/test_bench_launcher.py).

From 40 images of 416x416 (19 of 608x608) the Detector runs the batch as two sub-batches on two concurrent HIP streams
("lanes": same kernels and bits, each lane runs its own convolutions AND its own filter / NMS, so they fill each
other's idle CUs; --lanes 1 disables; the automatic lane count is a function of the batch shape, the same on every rank).  --batch is
images PER GPU (weak scaling, the default), --global-batch fixes the total (strong scaling; BASELINE configs[3] = 256
over 8).  Rank 0 prints ONE JSON line.

The HEADLINE (`value`, `dtype`, `roofline`) is the exact-fp32 mode (--dtype f32: fp32 in, fp32 accumulate, 24 significant bits =
the reference's arithmetic; round 6); the product's default 22-bit mode f32h2, the 24-bit f32x3 and bf16 are named
sub-objects of the same line with the same fields.

`roofline` is for the dominant kernel family, the convolutions behind the two fused front kernels (exact fp32:
conv_wino4_f32_kernel -- Winograd F(4x4,3x3) on v_mfma_f32_16x16x4_f32 -- and conv_igemm_f32_kernel; 71 launches per step): `achieved` /
`frac` = the matrix-instruction FLOPs those launches EXECUTE (a Winograd launch counts the multiplications of its form) divided by
the duration of their launch sequence, measured with HIP events on the launch stream in every timed step, against the dense MFMA
peak of the instruction's operand type (157.3 TFLOP/s fp32; 2500 for the 16-bit planes, whose fp32 product costs 3 or 6 MFMAs);
`algorithmic_tflops` / `algorithmic_frac` = the direct form's 2*MAC over the same time (above 1 where Winograd saves more than the
kernels lose).  Measured with ONE lane (the kernels alone on the chip); `roofline.two_lanes_section` is the rate of the
concurrent section as the timed step runs it (all 75 convs' FLOPs over the fork -> join wall time, which also contains the lanes'
filter + NMS).  A plain run whose timed step runs two lanes has no one-lane pass: its `roofline` holds `two_lanes_section` alone.

Extra objects on the same line, --full only (--no-extras skips them):
  cpu_baseline   the CPU oracle (oracle/oracle_cpu.py: the reference path restated in torch fp32 CPU ops) timed on this
                 box's host cores on bounded samples (416x416 bs=8, 608x608 bs=4, the dog image
                 bs=1; forward / decode / post-processing split);
  boxes_delta    "NMS boxes delta vs ref": the HIP path's final boxes vs the oracle's on the 416x416 sample;
  modes          the other math modes on the headline workload (f32h2, f32x3, bf16);
  configs        BASELINE.json configs by list index: "0" dog image bs=1 (GPU latency eager + HIP graph, CPU ms), "1",
                 "2", "3" (416x416, 256 images in total over the N GPUs of this run), "4", and eval mode at the reference's
                 0.005 / 0.45 ("eval": `Detector`; "eval_predict_and_process": the reference-shaped entry).
"""
import argparse
import glob
import json
import os
import socket
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch                       # noqa: E402
import torch.distributed as dist   # noqa: E402

# MI355X_MICROARCH.md dense MFMA peaks.  f32x3 / f32h2: every fp32 product costs six bf16 / three fp16 MFMAs, so the
# ceiling for ALGORITHMIC fp32 FLOP/s in those modes is 2500/6 and 2500/3 (frac == utilisation of the 16-bit matrix pipe).
PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0, "f32x3": 2500.0 / 6, "f32h2": 2500.0 / 3}
DTYPE_NAME = {"f32": "f32 (exact fp32 MFMA)", "bf16": "bf16 (fp32 accumulate)",
              "f32x3": "f32x3: fp32 emulated by an exact 3-way bf16 split (6 bf16 MFMAs per product, fp32 accumulate)",
              "f32h2": "f32h2: fp32 EMULATED by a 2-way fp16 split (22 significant bits, fp16 range; 3 fp16 MFMAs per product, fp32 accumulate)"}
MFMAS_PER_PRODUCT = {"f32": 1, "bf16": 1, "f32x3": 6, "f32h2": 3}
INSTR_PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0, "f32x3": 2500.0, "f32h2": 2500.0}   # dense peak of the MFMA the mode issues
KERNEL_NAME = {"f32": "conv_wino4_f32_kernel + conv_igemm_f32_kernel + conv_gemm1x1_f32_kernel", "bf16": "conv_planes_kernel<1>", "f32x3": "conv_planes_kernel<3>",
               "f32h2": "conv_planes_kernel<2> + conv_planes_w4_kernel"}
# kernels that make up the dominant family per mode (substring match on the rocprofv3 kernel names of the PMC child passes): the plane modes run the
# eight-wave / Winograd kernels of conv_planes.hip AND, since round 5, the four-wave two-workgroups-per-CU kernel of conv_planes_w4.hip
FAMILY = {"f32": ("conv_igemm_f32_kernel", "conv_wino4_f32_kernel", "conv_gemm1x1_f32_kernel"), "bf16": ("conv_planes_kernel", "conv_planes_w4_kernel"),
          "f32x3": ("conv_planes_kernel", "conv_planes_w4_kernel"), "f32h2": ("conv_planes_kernel", "conv_planes_w4_kernel")}
STAGES = ("conv0", "convs", "decode", "filter", "nms")


def usable_cores():
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def relaunch_under_torchrun(n, dry):
    """`python bench.py --gpus N` without a torchrun environment: become N ranks (one per GPU)."""
    if not dry and os.environ.get("YV3_DIST_BACKEND") != "gloo":
        have = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if have < n:
            sys.stderr.write("bench.py: --gpus %d needs %d visible GPUs (one rank per GPU over RCCL), found %d.  "
                             "(YV3_DIST_BACKEND=gloo rehearses the N-rank path on fewer GPUs: ranks then share devices "
                             "and gloo carries the gather -- functional check only, not a measurement.)\n" % (n, n, have))
            sys.exit(2)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    # a fresh child process, not exec: this process may already have initialised the GPU runtime (device count above)
    import subprocess
    sys.exit(subprocess.call(cmd, env=env))


def barrier(dev=None):
    """dist.barrier(); on the nccl (= RCCL) backend with this rank's device named explicitly -- without `device_ids` the first
    barrier of a process group GUESSES the device from the rank."""
    if dist.get_backend() == "nccl" and dev is not None and dev.type == "cuda":
        dist.barrier(device_ids=[dev.index if dev.index is not None else torch.cuda.current_device()])
    else:
        dist.barrier()


# ------------------------------------------------------------------------------------------------ CPU baseline
def _best(fn, reps=2):
    fn()                                                  # warm-up
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def cpu_baseline(stream, conf, nms, dog=None):
    """Oracle (CPU restatement of the reference path) on the host cores, as BASELINE.md section 4 plans it: 416x416 bs=8,
    608x608 bs=4 and the dog image bs=1; conv trunk / decode / post-processing timed separately (best of 2 after a
    warm-up each).  Returns (cpu_baseline object, the 416 sample, the oracle's boxes for it)."""
    from oracle import oracle_cpu as oc
    from yolo_v3_amd import synth
    cores = usable_cores()
    torch.set_num_threads(cores)
    sd, _ = oc.state_dict_from_stream(stream)
    samples = {}
    keep = None

    def run(tag, x):
        img_dim = (x.shape[3], x.shape[2])
        with torch.no_grad():
            t_trunk, logits = _best(lambda: oc.head_logits(sd, x))
            t_dec, dets = _best(lambda: torch.cat([oc.decode(l, oc.DEFAULT_ANCHORS, m, img_dim, 80)
                                                   for l, m in zip(logits, ((6, 7, 8), (3, 4, 5), (0, 1, 2)))], 1))
            t_pp, boxes = _best(lambda: oc.postprocess(dets.clone(), 80, conf, nms))
        n = x.shape[0]
        tot = t_trunk + t_dec + t_pp
        samples[tag] = {"images": n, "ms_per_img": {"conv_trunk": round(t_trunk / n * 1e3, 2), "decode": round(t_dec / n * 1e3, 3),
                                                    "postprocessing": round(t_pp / n * 1e3, 3), "total": round(tot / n * 1e3, 2)},
                        "images_per_sec": round(n / tot, 3)}
        return boxes

    x416 = torch.from_numpy(synth.images(8, 416, 1))
    keep = run("416x416_bs8", x416)
    run("608x608_bs4", torch.from_numpy(synth.images(4, 608, 2)))
    if dog is not None:
        run("dog_416x416_bs1", dog)
    obj = {"value": samples["416x416_bs8"]["images_per_sec"], "unit": "images/sec", "cores": cores, "kind": "port",
           "sample_short": "oracle on 8 images 416x416, best of 2",
           "sample": "oracle/oracle_cpu.py (torch fp32 CPU ops, %d threads), SW-1 weights: 8 images 416x416 (value), 4 images 608x608, "
                     "the letterboxed dog image; conv trunk, decode and post-processing timed separately, best of 2 after 1 warm-up" % cores,
           "samples": samples}
    return obj, x416, keep


# ------------------------------------------------------------------------------------------------ workloads
class Workload:
    """One (weights, batch, size, mode, thresholds) configuration measured through the product entry:
    `Detector.run_device` (world 1) / `ShardedDetector.run_device` (world > 1: + the one all-gather)."""

    def __init__(self, net, x, mode, conf, nms, is_eval=False, world=1, cap_host=512, max_cand=None, lanes=None):
        from yolo_v3_amd import Detector, _ffi
        from yolo_v3_amd import dist as ydist
        codes = {"f32": _ffi.F32, "bf16": _ffi.BF16, "f32x3": _ffi.F32X3, "f32h2": _ffi.F32H2}
        self.x, self.world, self.mode = x, world, mode
        B, _, H, W = x.shape
        self.B, self.size = B, H
        if world > 1:
            assert not is_eval
            self.sd = ydist.ShardedDetector(net, B, H, W, conf, nms, True, cap=cap_host, dtype=codes[mode], lanes=lanes)
            self.det = self.sd.det
            self.host = torch.empty((B * world, self.sd.cap + 1, 7), dtype=torch.float32).pin_memory()
        else:
            self.sd = None
            self.det = Detector(net, B, H, W, conf, nms, is_eval=is_eval, dtype=codes[mode], max_cand=max_cand, lanes=lanes)
            self.cap_host = min(self.det.cap, cap_host)
            self.host = torch.empty((B, self.cap_host, 7), dtype=torch.float32).pin_memory()
        self.host_counts = torch.empty((2 * B,), dtype=torch.int32).pin_memory()
        self.events = []
        self.gathered = None

    def step(self, timed):
        marks = {}

        def mark(name):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()                                   # on torch's current stream == the kernels' launch stream
            marks[name] = ev

        if self.sd is not None:
            self.gathered = self.sd.run_device(self.x, mark if timed else None)      # product code: conv0 ... NMS, pack, all-gather
            self.host.copy_(self.gathered, non_blocking=True)
        else:
            boxes, counts = self.det.run_device(self.x, mark if timed else None)     # product code: conv0 ... NMS
            self.host.copy_(boxes[:, :self.cap_host], non_blocking=True)
            self.host_counts.copy_(counts, non_blocking=True)
        if timed:
            mark("d2h")
            self.events.append(marks)

    def run(self, steps, warmup):
        def fence():
            if self.world > 1:
                barrier(self.x.device)
            torch.cuda.synchronize()
        with torch.no_grad():
            for _ in range(warmup):
                self.step(False)
            fence()
            t0 = time.perf_counter()
            for _ in range(steps):
                self.step(True)
            fence()
            elapsed = time.perf_counter() - t0
        self.own_elapsed = elapsed                                   # this rank's own clock (the reported time is the MAX over ranks)
        if self.world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device=self.x.device if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed

    def finish(self, rank=0):
        """Outside the timed region: what the product entry does with the result (list conversion = the one host
        sync; raises on a kernel status bit of ANY rank).  Returns (candidates, kept) of the first images."""
        if self.sd is not None:
            from yolo_v3_amd import dist as ydist
            spans = ydist.shard_plan(self.B, self.world, local_shard=True)[1]
            res = self.sd.assemble(self.gathered, spans)
            _, meta = ydist.unpack_payload(self.gathered)
            meta = meta.cpu()
            assert res == [] or len(res) == self.B * self.world
            return meta[:4, 0].tolist(), meta[:4, 1].tolist()
        self.det.engine.raise_if_overflowed(self.det.plan, int(self.det.plan.flags.item()))
        c = self.host_counts
        return c[:4].tolist(), c[self.B:self.B + 4].tolist()

    def last_outputs(self):
        """After `run` (it ends in a synchronise): (boxes, counts [B, 2], detections) of the LAST timed step -- the boxes and counts the
        caller of the timed entry receives (world 1: the host copies of `Detector.run_device`'s result; world > 1: the gathered payload
        of all ranks) and this rank's decoded detections."""
        if self.sd is not None:
            from yolo_v3_amd import dist as ydist
            boxes, meta = ydist.unpack_payload(self.gathered)
            return boxes, meta[:, :2], self.det.dets
        c = self.host_counts
        return self.host, torch.stack((c[:self.B], c[self.B:]), 1), self.det.dets

    def stages_ms(self):
        order = ["start"] + [s for s in STAGES] + (["gather"] if self.sd is not None else []) + ["d2h"]
        out = {}
        for prev, cur in zip(order, order[1:]):
            out[cur] = round(sum(m[prev].elapsed_time(m[cur]) for m in self.events) / len(self.events), 4)
        return out

    def flops(self):
        """(2*MAC of all 75 convs, 2*MAC of the launches timed as the 'convs' stage, number of those launches).
        One lane: the 'conv0' stage is the network's front (feature.mlist.0 alone, or -- fp16-plane mode -- the two fused
        front launches) and 'convs' the remaining implicit-GEMM launches.  Two lanes: 'convs' is the whole concurrent
        section (every conv launch of every lane, plus the lanes' filter + NMS)."""
        from yolo_v3_amd import arch
        specs = arch.conv_specs()
        hw = arch.conv_output_hw(self.size)
        macs = [h * w * sp.cout * sp.cin * sp.k * sp.k for sp, (h, w) in zip(specs, hw)]
        plan = self.det.plan
        first = 1 + plan.first_desc
        if self.det.lanes > 1:
            return 2.0 * sum(macs) * self.B, 2.0 * sum(macs) * self.B, sum(1 + (p.first_desc > 0) + (p.first_desc > 1) + p.n_desc - p.first_desc
                                                                         for p in self.det.lane_plans)
        return 2.0 * sum(macs) * self.B, 2.0 * sum(macs[first:]) * self.B, plan.n_desc - plan.first_desc

    def family_dispatches(self):
        """Kernel dispatches of the mode's dominant family per 'convs' stage of one lane: one per descriptor, two for an exact-fp32 1x1 layer that
        runs as persistent GEMM + small tiles (a Winograd launch's input transform is not in the family)."""
        p = self.det.plan
        return sum(1 if f != 0 else n for (_, f), n in zip(p.forms(), p.launches()))

    def algorithmic_bytes(self):
        """ALGORITHMIC HBM bytes of the launches timed as the 'convs' stage (one lane): every conv reads its input once, its
        residual once (second conv of a res_layer), its packed weights once and writes its output once.  Element size: 4 B in
        f32 / f32h2 (two fp16 planes), 6 B in f32x3, 2 B in bf16; head logits are fp32 in every mode; an upsample+concat input
        (768 / 384 channels) reads its upsampled part at the lower resolution.  DESIGN.md section 4."""
        from yolo_v3_amd import arch
        eb = {"f32": 4, "f32h2": 4, "f32x3": 6, "bf16": 2}[self.mode]
        specs = arch.conv_specs()
        hw = arch.conv_output_hw(self.size)
        first = 1 + self.det.plan.first_desc
        tot = 0
        for sp, (h, w) in list(zip(specs, hw))[first:]:
            hin, win = h * sp.stride, w * sp.stride
            if sp.cin in (768, 384):
                up = sp.cin // 3
                rd = (hin // 2) * (win // 2) * up + hin * win * (sp.cin - up)
            else:
                rd = hin * win * sp.cin
            out_b = h * w * sp.cout * (eb if sp.bn else 4)
            tot += self.B * (rd * eb + out_b + (out_b if sp.res2 else 0)) + sp.cout * sp.cin * sp.k * sp.k * eb
        return tot

    def form_bytes(self):
        """HBM bytes of the launches timed as the 'convs' stage IN THE FORM EACH ONE RUNS (exact-fp32 mode): a direct launch moves its
        algorithmic bytes; a Winograd launch additionally writes and reads back its transformed input V -- 16 values per 2x2 tile
        (F(2x2,3x3)) or 36 per 4x4 tile (F(4x4,3x3)) and channel, fp32 -- and reads the transformed filters (16/9 or 4x the 3x3 ones).
        `traffic / form_bytes` is then the re-read factor of the kernels themselves; `traffic / algorithmic_bytes` also contains the
        price of the form."""
        from yolo_v3_amd import arch
        if self.mode != "f32":
            return None
        specs = arch.conv_specs()
        tot = 0
        for p in self.det.lane_plans:
            for j, (si, f) in zip(range(p.first_desc, p.n_desc), p.forms()):
                d, sp = p.descs[j], specs[si]
                ho, wo = (d.H + 2 * ((sp.k - 1) // 2) - sp.k) // sp.stride + 1, (d.W + 2 * ((sp.k - 1) // 2) - sp.k) // sp.stride + 1
                if sp.cin in (768, 384):
                    up = sp.cin // 3
                    rd = (d.H // 2) * (d.W // 2) * up + d.H * d.W * (sp.cin - up)
                else:
                    rd = d.H * d.W * sp.cin
                out_b = ho * wo * sp.cout * 4
                wb = sp.cout * sp.cin * sp.k * sp.k * 4
                b = d.B * (rd * 4 + out_b + (out_b if sp.res2 else 0))
                if f == 1:
                    b += 2 * 16 * d.B * ((d.H + 1) // 2) * ((d.W + 1) // 2) * sp.cin * 4
                    wb = wb * 16 // 9
                elif f == 2:
                    b += 2 * 36 * d.B * ((d.H + 3) // 4) * ((d.W + 3) // 4) * sp.cin * 4
                    wb = wb * 4
                tot += b + wb
        return tot

    def executed(self):
        """EXECUTED matrix work of the launches timed as the 'convs' stage, next to the algorithmic (direct-form) count of
        `flops()`: (executed 2*MAC -- a launch that takes the Winograd F(2x2,3x3) form, as the library reports it through
        yv3_conv2d_form, counts 16 multiplications per 2x2 tile instead of 36 --, launches in the Winograd form, launches).
        Multiply by MFMAS_PER_PRODUCT[mode] for the matrix instructions' own FLOPs (split modes)."""
        from yolo_v3_amd import arch
        specs = arch.conv_specs()
        hw = arch.conv_output_hw(self.size)
        macs = [h * w * sp.cout * sp.cin * sp.k * sp.k for sp, (h, w) in zip(specs, hw)]
        ex, nw, nl = 0.0, 0, 0
        for p in self.det.lane_plans:
            fac = p.executed_mac_factor()
            forms = p.forms()
            for j, (si, f) in zip(range(p.first_desc, p.n_desc), forms):
                ex += 2.0 * macs[si] * p.descs[j].B * fac[si]
                nw += f != 0
                nl += 1
            if self.det.lanes > 1:                           # two lanes: the section also holds the front launches (direct form)
                ex += 2.0 * sum(macs[:1 + p.first_desc]) * p.B
        return ex, nw, nl

    def summary(self, elapsed, steps):
        st = self.stages_ms()
        fa, fi, nl = self.flops()
        ach = fi / (st["convs"] * 1e-3) / 1e12
        peak = PEAK_TFLOPS[self.mode]
        lanes = self.det.lanes
        ex, nwino, _ = self.executed()
        nwino4 = sum(f == 2 for p_ in self.det.lane_plans for _, f in p_.forms())
        ex_t = ex * MFMAS_PER_PRODUCT[self.mode] / (st["convs"] * 1e-3) / 1e12
        ipeak = INSTR_PEAK_TFLOPS[self.mode]
        return {"dtype": DTYPE_NAME[self.mode], "value": round(self.B * self.world * steps / elapsed, 2), "unit": "images/sec",
                "ms_per_step": round(elapsed / steps * 1e3, 4), "ms_per_img": round(elapsed / steps * 1e3 / (self.B * self.world), 5),
                "stages_ms": st, "lanes": lanes,
                "stages_note": ("one lane: consecutive stages on the launch stream" if lanes == 1 else
                                "%d lanes: 'convs' = fork -> join of the concurrent section (each lane: front, convs, filter, NMS on its own stream); "
                                "'decode' / 'filter' / 'nms' are inside it" % lanes),
                "roofline": {"bound": "mfma", "kernel": ("%s (%d launches/step)" % (KERNEL_NAME[self.mode], nl)) if lanes == 1 else
                             ("all conv launches of %d concurrent lanes (%d/step): FLOPs over the wall time of the concurrent section (incl. the lanes' filter + NMS)" % (lanes, nl)),
                             # round 6: `achieved` / `frac` are the EXECUTED matrix-instruction rate (never above 1); the
                             # algorithmic (direct-form) rate the contract's definition names stands beside it
                             "achieved": round(ex_t, 2), "peak": ipeak, "unit": "TFLOP/s", "frac": round(ex_t / ipeak, 4), "launches": nl,
                             "achieved_is": "EXECUTED rate: matrix-instruction FLOPs actually issued (a Winograd F(2x2,3x3) launch at 16/36 of its direct "
                                            "count, F(4x4,3x3) at 36/144, tile grids rounded up; x%d MFMAs per fp32 product in this mode) / the launches' "
                                            "time (HIP events), against the dense MFMA peak of the instruction's operand type" % MFMAS_PER_PRODUCT[self.mode],
                             "algorithmic_tflops": round(ach, 2), "algorithmic_peak": round(peak, 2), "algorithmic_frac": round(ach / peak, 4),
                             "algorithmic_is": "direct-convolution FLOPs (2*MAC, SURVEY 8d) of these launches / the same time: an EFFECTIVE rate wherever "
                                               "a launch runs a Winograd form -- above the peak when the forms save more than the kernels lose",
                             "winograd_launches": nwino, "winograd4_launches": nwino4,
                             "executed_tflops": round(ex_t, 2), "executed_peak": ipeak, "executed_frac": round(ex_t / ipeak, 4),
                             "all_75_convs_frac": round(fa / ((st["conv0"] + st["convs"]) * 1e-3) / 1e12 / peak, 4)}}


def make_net(stream, size, dev):
    from yolo_v3_amd import YoloNet, WeightManager
    net = YoloNet((size, size)).eval()
    assert WeightManager(net).load_stream(stream) == stream.size
    return net.to(dev)


def scenes(B, size, seed, dev, distinct=64):
    """B synthetic scenes; up to `distinct` different ones (default 64: every image of the headline batch differs -- the
    conv kernels' speed is data-dependent on this power-limited chip), tiled beyond that."""
    from yolo_v3_amd import synth
    base = synth.images(min(B, distinct), size, seed)
    return torch.from_numpy(base).to(dev).repeat((B + base.shape[0] - 1) // base.shape[0], 1, 1, 1)[:B].contiguous()


def attach_traffic(roof, dtype, size, B, n_desc):
    """HBM traffic of the dominant kernel family: FETCH_SIZE / WRITE_SIZE need their own rocprofv3 --pmc passes (they
    cannot be sampled from inside this process); the committed summary of those passes over THIS workload is attached
    and labelled with its source run (tools/traffic_summary.py -> profiles/*_traffic_<dtype>_<size>_bs<B>.json)."""
    cands = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_traffic_%s_%d_bs%d.json" % (dtype, size, B))))
    roof["traffic"] = None
    if not cands:
        return
    fam = json.load(open(cands[-1])).get(KERNEL_NAME[dtype].split("<")[0])
    if fam:
        roof["traffic"] = round(fam["hbm_bytes_per_step_fetch_x2"] / n_desc)
        roof["traffic_source"] = os.path.basename(cands[-1])
        roof["traffic_note"] = ("HBM bytes per launch (avg of %d launches/step) = (2*FETCH_SIZE + WRITE_SIZE)*1024 from separate "
                                "rocprofv3 --pmc passes of this workload, NOT measured in this run; FETCH_SIZE doubled per the "
                                "gfx950 calibration in MI355X_MICROARCH.md" % n_desc)


def _in_family(kernel_name, family):
    """`family`: one substring or a tuple of them (a kernel belongs when its name contains any)."""
    return any(f in kernel_name for f in ((family,) if isinstance(family, str) else family))


def sum_counter(csv_path, family, counter=None):
    """(sum of Counter_Value, number of dispatches) over the kernels of `family` in a rocprofv3 counter_collection.csv
    (`counter`: only rows of that counter, for passes that collect several)."""
    import csv
    per = {}
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            if _in_family(r["Kernel_Name"], family) and (counter is None or r["Counter_Name"] == counter):
                per[r["Dispatch_Id"]] = per.get(r["Dispatch_Id"], 0.0) + float(r["Counter_Value"])
    return sum(per.values()), len(per)


def family_wall_ns(trace_csv, family):
    """Sum of End - Start over the kernels of `family` in a rocprofv3 kernel_trace.csv."""
    import csv
    tot = 0
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            if _in_family(r["Kernel_Name"], family):
                tot += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    return tot


LIVE_TRAFFIC = {"ok": True}          # one failed pass (missing tool, time-out, crash) switches the live measurement off for the rest of the run


def live_traffic(roof, args, B, timeout_s=60, dtype=None, size=None, weights=None, conf=None, nms=None, dispatches_per_launch=1.0):
    """HBM bytes per launch of the dominant kernel family, measured for THIS binary on THIS box: two rocprofv3 --pmc passes
    (FETCH_SIZE, WRITE_SIZE -- separate passes, as MI355X_MICROARCH.md prescribes) over a 3-step one-lane run of the same
    workload in child processes (counters cannot be sampled from inside this process).  traffic = (2*FETCH + WRITE) * 1024 /
    launches: KiB units, FETCH_SIZE doubled per the guide's gfx950 calibration.  A third pass of the same kind
    (SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE) gives the matrix pipe's measured utilisation and the effective clock of
    the same launches (`mfma_util`, `clock_ghz`).  Returns False (and leaves `roof` alone) when
    rocprofv3 is missing or a traffic pass fails; the caller then attaches the committed summary instead."""
    import shutil
    import subprocess
    import tempfile
    if not LIVE_TRAFFIC["ok"]:
        roof["traffic_live_error"] = "switched off after an earlier failure in this run"
        return False
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        roof["traffic_live_error"] = "rocprofv3 not found"
        LIVE_TRAFFIC["ok"] = False
        return False
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ) or "rocprofiler" in os.environ.get("LD_PRELOAD", ""):
        roof["traffic_live_error"] = "this process is itself being profiled"
        return False
    dtype, size, weights = dtype or args.dtype, size or args.size, weights or args.weights
    conf, nms = args.conf if conf is None else conf, args.nms if nms is None else nms
    fam = FAMILY[dtype]
    sums = {}
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    t0 = time.time()
    for ctr in ("FETCH_SIZE", "WRITE_SIZE", "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE"):
        d = tempfile.mkdtemp(prefix="yv3_pmc_", dir="/tmp")
        cmd = [exe, "--pmc"] + ctr.split() + ["--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--", sys.executable,
               os.path.abspath(__file__), "--lanes", "1", "--steps", "3",                  # a plain run: the headline steps alone
               "--warmup", "1", "--batch", str(B), "--size", str(size), "--dtype", dtype, "--weights", weights,
               "--conf", str(conf), "--nms", str(nms)]
        try:
            # own session: on a time-out the whole group (rocprofv3 AND the python it started) is killed, nothing keeps the GPU busy
            proc = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
            try:
                proc.wait(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                import signal
                os.killpg(proc.pid, signal.SIGKILL)
                proc.wait()
                raise
            if proc.returncode != 0:
                raise subprocess.CalledProcessError(proc.returncode, cmd[0])
            hits = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if " " in ctr:                                         # the matrix-pipe pass: busy cycles, chip-active cycles, wall time
                tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
                sums["MFMA"] = (sum_counter(hits[0], fam, "SQ_VALU_MFMA_BUSY_CYCLES")[0], sum_counter(hits[0], fam, "GRBM_GUI_ACTIVE")[0],
                                family_wall_ns(tr[0], fam))
            else:
                sums[ctr] = sum_counter(hits[0], fam)
        except Exception as e:                                     # noqa: BLE001 -- any failure means "use the committed summary"
            if " " in ctr and "FETCH_SIZE" in sums and "WRITE_SIZE" in sums:
                roof["mfma_util_live_error"] = "%s pass: %s" % (ctr, type(e).__name__)      # the traffic passes stand
                break
            roof["traffic_live_error"] = "%s pass: %s" % (ctr, type(e).__name__)
            LIVE_TRAFFIC["ok"] = False
            return False
        finally:
            shutil.rmtree(d, ignore_errors=True)
    (f, nf), (w, nw) = sums["FETCH_SIZE"], sums["WRITE_SIZE"]
    if nf == 0 or nf != nw:
        roof["traffic_live_error"] = "dispatch counts differ (%d / %d)" % (nf, nw)
        return False
    if "MFMA" in sums and sums["MFMA"][1] > 0 and sums["MFMA"][2] > 0:
        busy, gui, wall = sums["MFMA"]
        cyc = gui / 8.0                                            # GRBM_GUI_ACTIVE is summed over the 8 XCDs
        roof["mfma_util"] = round(busy / (cyc * 1024), 4)          # SQ_VALU_MFMA_BUSY_CYCLES is summed over the chip's 1024 SIMDs
        roof["clock_ghz"] = round(cyc / wall, 3)
        roof["mfma_util_note"] = ("PMC, third child pass of the same one-lane workload: SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE/8 * 1024 SIMDs) "
                                  "over the launches of %s; clock = GRBM_GUI_ACTIVE/8 / their wall time (2.4 GHz nominal: the matrix pipe's "
                                  "share of the nominal peak is mfma_util * clock_ghz / 2.4)" % " + ".join(fam))
    roof["traffic"] = round((2 * f + w) * 1024 / nf * dispatches_per_launch)     # per LAUNCH of the roofline object (= per descriptor)
    roof["traffic_source"] = "measured in this run"
    roof["traffic_note"] = ("HBM bytes per launch = (2*FETCH_SIZE + WRITE_SIZE)*1024 / %d profiled launches of %s: rocprofv3 --pmc "
                            "passes (one counter each; a third pass for the matrix pipe) over 3 one-lane steps of this workload in child processes, %.0f s; FETCH_SIZE "
                            "doubled per the gfx950 calibration in MI355X_MICROARCH.md; algorithmic bytes per launch: flop-independent, "
                            "see DESIGN.md section 3" % (nf, " + ".join(fam), time.time() - t0))
    return True


def _pick(d, keys, rename=None):
    """{k: d[k]} for the keys present (numbers / short strings only), optionally renamed."""
    rename = rename or {}
    return {rename.get(k, k): d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


ROOF_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "algorithmic_tflops", "algorithmic_frac", "executed_tflops", "executed_frac",
             "mfma_util", "clock_ghz", "traffic", "algorithmic_bytes", "form_bytes", "launches", "winograd_launches", "winograd4_launches",
             "avg_launch_ms", "conv_ms_per_step")
MODE_ROOF_KEYS = ("achieved", "peak", "frac", "algorithmic_frac", "mfma_util", "clock_ghz", "traffic", "algorithmic_bytes", "launches",
                  "winograd_launches")


def compact_line(out, full_path=None):
    """The ONE line the driver parses (contract: < 4 KB): numbers and short labels only.  Everything else -- per-mode and per-config
    objects, the per-rank table, the PCIe-inclusive passes, every explanatory note -- is in the full object (`full`); what the fields
    mean is DESIGN.md section 8."""
    c = {k: out[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_img", "higher_is_better",
                             "scaling", "vs_baseline", "dtype", "data") if k in out}
    c["config"] = _pick(out.get("config", {}), ("workload", "global_batch", "parallelism", "entry", "collective", "backend"))
    if "lanes" in out:
        c["config"]["lanes"] = out["lanes"]
    if "stages_ms_one_lane" in out:
        c["stages_ms_one_lane"] = out["stages_ms_one_lane"]
    if "ok" in out:
        c["ok"] = out["ok"]
    if "roofline" in out:
        r = _pick(out["roofline"], ROOF_KEYS)
        if "kernel" in r:
            r["kernel"] = r["kernel"].split(" (")[0]
        two = out["roofline"].get("two_lanes_section")
        if two:
            r["two_lanes"] = _pick(two, ("achieved", "frac", "executed_frac"))
        c["roofline"] = r
    if "cpu_baseline" in out:
        cb = out["cpu_baseline"]
        c["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind"))
        c["cpu_baseline"]["sample"] = cb.get("sample_short") or str(cb.get("sample", ""))[:60]
    if "boxes_delta" in out:
        c["boxes_delta"] = _pick(out["boxes_delta"], ("images", "ref_boxes", "got_boxes", "matched_iou_ge_0.999", "max_rel_err_coords", "tolerance"),
                                 {"ref_boxes": "ref", "got_boxes": "got", "matched_iou_ge_0.999": "matched", "max_rel_err_coords": "max_rel_err"})
    modes = out.get("modes", {})
    for key, mode in (("exact_f32", "f32"), ("f32h2", "f32h2"), ("bf16", "bf16"), ("f32x3", "f32x3")):
        if mode in modes:
            m = modes[mode]
            c[key] = dict(_pick(m, ("value", "ms_per_step")), **_pick(m.get("roofline", {}), MODE_ROOF_KEYS))
    cfgs = out.get("configs", {})
    if cfgs:
        c["configs"] = {}
        for k, v in cfgs.items():
            if k == "0":
                c["configs"][k] = _pick(v, ("gpu_ms_per_img", "boxes"))
            else:
                c["configs"][k] = dict(_pick(v, ("value", "ms_per_step", "lanes")), **_pick(v.get("roofline", {}), ("frac", "algorithmic_frac")))
    pc = out.get("pcie_inclusive", {})
    if "double_buffered" in pc:
        c["pcie_inclusive"] = {"serial": pc.get("serial", {}).get("images_per_sec"), "double_buffered": pc["double_buffered"]["images_per_sec"]}
    if "ranks" in out and len(out["ranks"]) > 1:
        c["ranks"] = [_pick(r, ("rank", "lanes", "own_ms_per_step")) for r in out["ranks"]]
    if full_path:
        c["full"] = full_path
    return c


def write_full(out, args):
    """The full result object as a side file (gpurun_out/ is merged back from the GPU box); returns its repo-relative path."""
    try:
        d = os.path.join(REPO, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        name = "bench_full.json" if out.get("n_gpus", 1) == 1 else "bench_full_%dgpu.json" % out["n_gpus"]
        with open(os.path.join(d, name), "w") as f:
            json.dump(out, f)
        return "gpurun_out/" + name
    except OSError:
        return None


DUMP_LIMIT_BYTES = 64 * 10 ** 6       # --dump-outputs: all files together (64 MB)
DUMP_SAMPLE_SEED = 0                 # fixed row sample of the decoded detections


def dump_outputs(d, boxes, counts, dets):
    """--dump-outputs DIR: what the timed path computed in its last step, as .npy files, so that two builds run with the same
    arguments (hence the same seeded weights and scenes) can be compared output for output.  Tensors in (any device):
      boxes [B, cap, 7] fp32 (the final boxes), counts [B, 2] (candidates, kept per image), dets [B, N, A] fp32 (the decoded detections
      the filter / NMS read).  Files out:
      boxes.npy              float32 [B, cap, 7]  rows past an image's kept count are zeroed (they are not part of the result)
      counts.npy             float64 [B, 2]       candidates, kept
      detections_sample.npy  float32 [B, R, A]    the same R rows of every image (seeded sample, sorted; all rows when they fit)
      detection_rows.npy     float64 [R]          ... their row indices
    Together at most DUMP_LIMIT_BYTES.  Returns {name: bytes}."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    counts = counts.cpu().to(torch.float64).numpy()
    kept = counts[:, 1].astype(np.int64)
    bx = boxes.cpu().to(torch.float32).numpy().copy()
    bx[np.arange(bx.shape[1])[None, :] >= kept[:, None]] = 0.0
    B, N, A = dets.shape
    room = DUMP_LIMIT_BYTES - bx.nbytes - counts.nbytes - (1 << 20)      # (1 MiB for the row indices and the .npy headers)
    R = int(min(N, max(1, room // (B * A * 4))))
    rows = np.arange(N) if R == N else np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(N, size=R, replace=False))
    sample = dets[:, torch.from_numpy(rows).to(dets.device)].cpu().to(torch.float32).numpy()
    files = {"boxes": bx, "counts": counts, "detections_sample": sample,
             "detection_rows": rows.astype(np.float64)}
    sizes = {}
    for name, a in files.items():
        np.save(os.path.join(d, name + ".npy"), a)
        sizes[name] = a.nbytes
    assert sum(sizes.values()) <= DUMP_LIMIT_BYTES, sizes
    return sizes


def dry_run(args, rank, world):
    """Launcher / rendezvous / collective / JSON-line rehearsal on CPU tensors: every rank builds a synthetic payload
    with the PRODUCT's pack function, runs the product's single all-gather K times (barrier + max-over-ranks timing as
    the real run) and assembles the global result.  No GPU, no kernels, no throughput claim."""
    from yolo_v3_amd import dist as ydist
    B, cap = 4, 8
    lo, _ = ydist.shard_range(B * world, rank, world)
    boxes = torch.zeros(B, cap, 7)
    kept = torch.tensor([(lo + i) % 3 for i in range(B)], dtype=torch.int32)
    for i in range(B):
        boxes[i, :int(kept[i]), 0] = float(lo + i)
    payload = ydist.pack_payload(boxes, kept, kept, torch.zeros(1, dtype=torch.int32))
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gathered = ydist.gather_payload(payload)
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    spans = ydist.shard_plan(B, world, local_shard=True)[1]
    res, status = ydist.assemble_global(gathered, spans, B, max_cand=cap)
    ok = status == 0 and len(res) == B * world and all((r.shape[0] if r.numel() else 0) == g % 3 for g, r in enumerate(res))
    if rank == 0:
        print(json.dumps(compact_line({"metric": "dry run: launcher + pack/gather/assemble on CPU tensors (no kernels)", "value": None, "unit": "images/sec",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 4),
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "n/a", "data": "dry-run",
                          "config": {"workload": "dry run", "global_batch": B * world, "parallelism": "dp%d" % world,
                                     "backend": dist.get_backend() if world > 1 else None}, "ok": bool(ok)}), separators=(",", ":")))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    sys.exit(0 if ok else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU per step (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=0, help="total images per step, split over the GPUs (strong scaling)")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--dtype", default="f32", choices=["f32", "f32x3", "f32h2", "bf16"],
                    help="conv math mode of the HEADLINE; default f32 = exact fp32 MFMA (24 significant bits: the reference's arithmetic).  f32h2 "
                         "(22-bit fp16 split, the product's default mode), f32x3 (24-bit bf16 split) and bf16 are reported as named sub-objects; "
                         "f32, f32x3 and f32h2 all meet the 1e-4 fp32 parity bar (tests/test_gpu_e2e.py)")
    ap.add_argument("--conf", type=float, default=0.5)
    ap.add_argument("--nms", type=float, default=0.4)
    ap.add_argument("--lanes", type=int, default=0, help="sub-batches run concurrently on separate HIP streams (0 = Detector's default: "
                    "2 when it measures a gain on this GPU, else 1)")
    ap.add_argument("--full", action="store_true", help="besides the headline, measure and check everything else: the one-lane roofline "
                    "pass, the rocprofv3 --pmc passes, the other modes and configs, the PCIe passes, the CPU baseline and boxes_delta "
                    "(about two minutes); the full object also goes to a side file, named by the line's `full`")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the extra modes / configs measurements")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and boxes_delta")
    ap.add_argument("--no-live-traffic", action="store_true", help="with --full: do not run the rocprofv3 --pmc passes for roofline.traffic "
                    "(~1 min, N=1 only); attach the committed summary of such passes instead")
    ap.add_argument("--full-line", action="store_true", help="also print the result object (with --full: modes, configs, per-rank table, "
                    "notes; ~20 KB) as an earlier stdout line")
    ap.add_argument("--dry-run", action="store_true", help="launcher + collective rehearsal on CPU tensors (no GPU needed)")
    ap.add_argument("--weights", default="sw1", choices=["sw1", "dense", "eval"],
                    help="sw1: ~50-150 candidates/img; dense: ~1e4 rows/img pass conf (BASELINE configs[4]); eval: SW-eval")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last one computed to DIR/*.npy "
                    "(final boxes, counts, a fixed sample of the decoded detections; float32 / float64, <= 64 MB; see dump_outputs)")
    args = ap.parse_args()

    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1")
    if not args.full:                          # a plain run: the headline alone, every extra measurement is --full's
        args.no_extras = args.no_cpu_baseline = args.no_live_traffic = True
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        relaunch_under_torchrun(args.gpus, args.dry_run)              # does not return
    if env_world is not None and int(env_world) != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%s: launch one rank per GPU (`python bench.py --gpus N` does it itself, or "
                         "`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`)\n" % (args.gpus, env_world))
        sys.exit(2)

    from yolo_v3_amd import synth, dist as ydist

    rank, local, world = ydist.init_from_env(backend="gloo" if args.dry_run else None)
    if args.dry_run:
        dry_run(args, rank, world)
    if not torch.cuda.is_available():
        sys.stderr.write("bench.py needs the MI355X (there is no CPU path)\n")
        sys.exit(2)
    dev = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(dev)

    t_proc = time.perf_counter()
    strong = args.global_batch > 0
    if strong:
        if args.global_batch % world:
            sys.stderr.write("--global-batch must be a multiple of the number of GPUs\n")
            sys.exit(2)
        B = args.global_batch // world
    else:
        B = args.batch
    streams = {"sw1": synth.weight_stream, "dense": synth.dense_weight_stream, "eval": synth.eval_weight_stream}
    stream = streams[args.weights]()
    net = make_net(stream, args.size, dev)
    lo, _ = ydist.shard_range(B * world, rank, world)
    x = scenes(B, args.size, 1000 + lo, dev)

    t_setup = time.perf_counter() - t_proc                            # weights generated + loaded, scenes resident
    # Workload construction holds NO collective (round 5: the lane count is a function of the batch shape); the time a rank spends
    # before and inside the constructor (packing, stream probe) is reported per rank below
    main_w = Workload(net, x, args.dtype, args.conf, args.nms, world=world, lanes=args.lanes or None)
    t_build = time.perf_counter() - t_proc - t_setup
    elapsed = main_w.run(args.steps, args.warmup)
    cand4, kept4 = main_w.finish(rank)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, *main_w.last_outputs())     # before anything else runs the Detector again
    rank_info = {"rank": rank, "device": str(dev), "lanes": main_w.det.lanes,
                 "setup_s": round(t_setup, 2), "detector_build_s": round(t_build, 2),
                 "own_ms_per_step": round(main_w.own_elapsed / args.steps * 1e3, 4)}
    ranks = [rank_info]
    if world > 1:
        ranks = [None] * world
        dist.all_gather_object(ranks, rank_info)                      # (after the timed region; every rank takes part)
    if rank == 0 and os.environ.get("YV3_DUMP_PLAN"):               # for tools/trace_layers.py: conv spec index of every launch
        p_ = main_w.det.plan
        json.dump({"first_desc": p_.first_desc, "desc_spec": p_.desc_spec, "desc_launches": p_.launches()}, open(os.environ["YV3_DUMP_PLAN"], "w"))
    head = main_w.summary(elapsed, args.steps)

    sub_steps, sub_warm = 10, 3
    cfg3 = None
    if not args.no_extras:
        # ---- BASELINE configs[3]: 416x416, 256 images in total, sharded over the GPUs of THIS run (every rank takes part)
        if 256 % world == 0 and not (strong and args.global_batch == 256 and args.size == 416):
            b3 = 256 // world
            lo3, _ = ydist.shard_range(256, rank, world)
            net416 = net if args.size == 416 and args.weights == "sw1" else make_net(synth.weight_stream(), 416, dev)
            w3 = Workload(net416, scenes(b3, 416, 3000 + lo3, dev), args.dtype, 0.5, 0.4, world=world, lanes=args.lanes or None)
            e3 = w3.run(sub_steps, sub_warm)
            c3, k3 = w3.finish(rank)
            if rank == 0:
                s3 = w3.summary(e3, sub_steps)
                s3["workload"] = ("BASELINE configs[3]: 416x416, global batch 256 sharded over %d GPU(s) (%d per GPU), RCCL box gather; "
                                  "the config names 8 GPUs" % (world, b3))
                s3["kept_per_img_first4"], s3["candidates_per_img_first4"] = k3, c3
                cfg3 = s3
            del w3, net416
            torch.cuda.empty_cache()

    # The roofline of the dominant KERNEL is measured with the kernels running alone (one lane): with two concurrent lanes a
    # kernel's duration includes the time it shares the chip with the other lane's kernels (rocprofv3 then shows per-kernel
    # durations that sum to ~2x the wall time).  The two-lane section rate (FLOPs over wall) is reported next to it.
    lanes_used = main_w.det.lanes
    roof_w, head1 = main_w, head
    if lanes_used > 1 and rank == 0 and args.full:
        # rank-local (world=1: no collective inside) and placed AFTER the last collective-bearing section of the run (configs "3"
        # above): the other ranks wait for rank 0 only in the final barrier, never inside a data-path collective
        roof_w = Workload(net, x, args.dtype, args.conf, args.nms, world=1, lanes=1)
        e1 = roof_w.run(min(args.steps, 10), 3)
        head1 = roof_w.summary(e1, min(args.steps, 10))
    out = None
    if rank == 0:
        out = {
            "metric": "images/sec (YOLOv3 forward + decode + NMS, %dx%d, bs=%d per GPU)" % (args.size, args.size, B),
            "value": head["value"], "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"], "ms_per_img": head["ms_per_img"],
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": DTYPE_NAME[args.dtype], "data": "synthetic",
            "config": {"workload": "%dx%d bs=%d per GPU, %d distinct synthetic scenes per GPU, %s synthetic weights, conf=%.2f nms=%.2f"
                                   % (args.size, args.size, B, min(B, 64), {"sw1": "SW-1", "dense": "SW-dense", "eval": "SW-eval"}[args.weights],
                                      args.conf, args.nms),
                       "global_batch": B * world, "parallelism": "dp%d" % world,
                       "entry": "ShardedDetector.run_device (= detect_sharded without the list conversion)" if world > 1 else "Detector.run_device",
                       "collective": ("1 x all_gather_into_tensor of [%d, %d, 7] fp32 per rank, backend %s" % (B, main_w.sd.cap + 1, dist.get_backend()))
                       if world > 1 else None,
                       "candidates_first_images": cand4, "boxes_kept_first_images": kept4},
            "stages_ms": head["stages_ms"], "stages_note": head["stages_note"], "lanes": lanes_used, "roofline": {},
        }
        if roof_w.det.lanes == 1:                # (a plain run whose timed step runs two lanes has no one-lane pass)
            fa, fi, n_desc = roof_w.flops()
            alg_bytes = roof_w.algorithmic_bytes()
            st = head1["stages_ms"]
            # the per-stage split that means what it says: consecutive stages of the ONE-lane pass (under two lanes everything from the
            # fork to the join is one concurrent section and the later marks are event order, not stage cost)
            out["stages_ms_one_lane"] = head1["stages_ms"]
            out["roofline"] = dict(head1["roofline"], traffic=None,
                                   algorithmic_bytes=round(alg_bytes / n_desc),
                                   **({"form_bytes": round(roof_w.form_bytes() / n_desc)} if args.dtype == "f32" else {}),
                                   conv_ms_per_step=st["convs"], avg_launch_ms=round(st["convs"] / n_desc, 5),
                                   flop_per_launch_avg=fi / n_desc,
                                   end_to_end_frac=round(fa / (head["ms_per_step"] * 1e-3) / 1e12 / PEAK_TFLOPS[args.dtype], 4))
            if lanes_used > 1:
                out["roofline"]["measured_with"] = ("lanes=1 (%.2f images/s, %.3f ms/step): the kernels run alone, so HIP-event and rocprofv3 per-kernel "
                                                    "durations mean what they say; the timed step above runs %d concurrent lanes"
                                                    % (head1["value"], head1["ms_per_step"], lanes_used))
            if args.no_live_traffic or world > 1 or not live_traffic(out["roofline"], args, B, dispatches_per_launch=roof_w.family_dispatches() / n_desc):
                attach_traffic(out["roofline"], args.dtype, args.size, B, n_desc)
            if args.dtype in ("f32x3", "f32h2"):
                nm = {"f32x3": 6, "f32h2": 3}[args.dtype]
                out["roofline"]["note"] = ("achieved = matrix-instruction FLOP/s issued (%d MFMAs per fp32 product) against the 2500 TFLOP/s dense 16-bit "
                                           "peak; algorithmic_* = fp32 FLOP/s of the direct form against 2500 / %d; mfma_util / clock_ghz are the PMC reading"
                                           % (nm, nm))
                out["roofline"]["frac_vs_fp32_mfma_peak"] = round(out["roofline"]["algorithmic_tflops"] / PEAK_TFLOPS["f32"], 4)
        if lanes_used > 1:
            out["roofline"]["two_lanes_section"] = {k: head["roofline"][k] for k in ("kernel", "achieved", "frac", "algorithmic_tflops", "algorithmic_frac",
                                                                                  "launches", "winograd_launches", "winograd4_launches")}
        if cfg3 is not None:
            out.setdefault("configs", {})["3"] = cfg3
        out["ranks"] = ranks
        out["ranks_note"] = ("per rank: lanes the Detector runs (a function of the batch shape + a yes/no stream-concurrency probe; no collective "
                             "in the constructor), seconds before / inside the Detector constructor, and its OWN clock over the timed "
                             "steps (ms_per_step above is the MAX over ranks)")
    del roof_w

    extras = world == 1 and not args.no_extras and rank == 0
    if extras:
        # ---- the other math modes on the headline workload (driver-timed, same entry point)
        out["modes"] = {}
        # (+ bf16: REDUCED precision -- conv operands rounded to bfloat16 as in BASELINE configs[2]; not a parity mode)
        for mode in ("f32h2", "f32x3", "f32", "bf16"):
            if mode == args.dtype:
                continue
            w = Workload(net, x, mode, args.conf, args.nms)
            out["modes"][mode] = w.summary(w.run(sub_steps, sub_warm), sub_steps)
            w.finish()
            out["modes"][mode]["roofline"]["algorithmic_bytes"] = round(w.algorithmic_bytes() / out["modes"][mode]["roofline"]["launches"])
            if args.no_live_traffic or world > 1 or not live_traffic(out["modes"][mode]["roofline"], args, B, dtype=mode):
                attach_traffic(out["modes"][mode]["roofline"], mode, args.size, B, out["modes"][mode]["roofline"]["launches"])
            if mode == "bf16":
                out["modes"][mode]["note"] = "reduced precision (bf16 conv operands, fp32 accumulate / epilogue / decode): outside the 1e-4 parity bar"
            del w
        # ---- BASELINE.json configs (list indices): 1 = 416 bs32 fp32; 2 = 608 bs16 bf16 convs; 4 = 608 bs8 dense scene
        out.setdefault("configs", {})

        def sub(key, label, net_, x_, mode, conf, nms, **kw):
            w = Workload(net_, x_, mode, conf, nms, **kw)
            s = w.summary(w.run(sub_steps, sub_warm), sub_steps)
            s["workload"] = label
            s["candidates_per_img_first4"], s["kept_per_img_first4"] = w.finish()
            wname = {"1": "sw1", "2": "sw1", "4": "dense"}.get(key)          # (live PMC passes for the BASELINE configs only)
            live = wname is not None and not args.no_live_traffic and world == 1 and live_traffic(
                s["roofline"], args, x_.shape[0], dtype=mode, size=x_.shape[2], weights=wname, conf=conf, nms=nms)
            if not live:
                attach_traffic(s["roofline"], mode, x_.shape[2], x_.shape[0], s["roofline"]["launches"])
            out["configs"][key] = s

        ref_mode = args.dtype if args.dtype in ("f32", "f32x3") else "f32"      # BASELINE "fp32" configs run a >= 24-bit arithmetic
        sub("1", "416x416 bs=32 SW-1 fp32 (%s) conf=0.5 nms=0.4" % ref_mode, net, scenes(32, 416, 1, dev), ref_mode, 0.5, 0.4)
        sub("1_f32h2", "416x416 bs=32 SW-1, the product's default 22-bit mode f32h2, conf=0.5 nms=0.4", net, scenes(32, 416, 1, dev), "f32h2", 0.5, 0.4)
        net608 = make_net(stream, 608, dev)
        sub("2", "608x608 bs=16 SW-1 bf16 convs / fp32 decode conf=0.5 nms=0.4", net608, scenes(16, 608, 2, dev), "bf16", 0.5, 0.4)
        del net608
        dnet = make_net(synth.dense_weight_stream(), 608, dev)
        sub("4", "608x608 bs=8 SW-dense (>=5k pre-NMS rows/img) %s conf=0.5 nms=0.4" % ref_mode, dnet, scenes(8, 608, 4, dev), ref_mode, 0.5, 0.4,
            cap_host=8192)
        del dnet
        enet = make_net(synth.eval_weight_stream(), 416, dev)
        xe = scenes(32, 416, 5, dev)
        sub("eval", "416x416 bs=32 SW-eval, eval mode as evaluate.py:201-204 (conf=0.005 nms=0.45 is_eval=True), Detector.run_device", enet,
            xe, ref_mode, 0.005, 0.45, is_eval=True, cap_host=4096, max_cand=8192)
        # the reference-shaped eval entry: evaluate.predict_and_process -> detect(is_eval=True) -> list of CPU tensors per batch
        from yolo_v3_amd import evaluate as yeval

        class CountBoxes(yeval.BatchHandler):
            n = 0

            def process_batch(self, sample, predictions):
                CountBoxes.n += sum(int(p.shape[0]) for p in predictions if p.numel())

        sample = {"img": xe, "org_img": [None] * 32, "img_path": ["%d.jpg" % i for i in range(32)]}
        yeval.predict_and_process([sample] * 2, enet, 80, CountBoxes())                       # warm-up (buffers, lane calibration)
        torch.cuda.synchronize()
        CountBoxes.n = 0
        t0 = time.perf_counter()
        yeval.predict_and_process([sample] * sub_steps, enet, 80, CountBoxes())
        torch.cuda.synchronize()
        te = time.perf_counter() - t0
        out["configs"]["eval_predict_and_process"] = {
            "workload": "the same 32 images through evaluate.predict_and_process (reference evaluate.py:197-206): detect(is_eval=True) + list of "
                        "per-image CPU tensors handed to a batch handler, %d batches" % sub_steps,
            "value": round(32 * sub_steps / te, 2), "unit": "images/sec", "ms_per_step": round(te / sub_steps * 1e3, 4),
            "boxes_per_batch": CountBoxes.n // sub_steps}
        del enet, xe
        torch.cuda.empty_cache()

    if rank == 0 and world == 1 and not args.no_extras:
        # ---- the headline step with the batch handed over as a HOST buffer (the reference's test.py builds its batch on the host
        # and calls .cuda(): /root/reference test.py:28-34).  Never `value` -- the C-ABI takes device pointers -- but what a caller
        # of `detect(net, host_batch)` sees: (a) serial: H2D copy, then the step; (b) double-buffered: the copy of batch i+1 on a
        # copy stream under the step of batch i; (c) uint8 HWC frames (4x fewer bytes over PCIe) converted on the GPU.
        def pcie_inclusive():
            xh = main_w.x.detach().cpu().pin_memory()
            nb = xh.numel() * xh.element_size()
            n = min(args.steps, 10)
            xd = [torch.empty_like(main_w.x), torch.empty_like(main_w.x)]
            res = {"batch_bytes_f32": nb}
            with torch.no_grad():
                for _ in range(2):
                    xd[0].copy_(xh, non_blocking=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    xd[0].copy_(xh, non_blocking=True)
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) / n
                res["h2d_ms"], res["h2d_GBps"] = round(t * 1e3, 3), round(nb / t / 1e9, 1)
                t0 = time.perf_counter()
                xd[0].copy_(xh, non_blocking=True)
                res["h2d_call_blocks_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)      # (an asynchronous call returns in microseconds)
                torch.cuda.synchronize()
                keep_x = main_w.x
                # (a) serial
                main_w.x = xd[0]
                for it in range(2 + n):
                    if it == 2:
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                    xd[0].copy_(xh, non_blocking=True)
                    main_w.step(False)
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) / n
                res["serial"] = {"ms_per_step": round(t * 1e3, 3), "images_per_sec": round(B / t, 1)}
                # (b) double-buffered: copy of batch i+1 on a copy stream while batch i is processed.  HIP maps streams onto a few hardware
                # queues and two streams on the same queue serialise (yolo_v3_amd/detect.py, lanes): several fresh streams are tried and
                # the best is kept -- what an integrator's input pipeline would do once at start-up.
                cur = torch.cuda.current_stream(dev)
                ready = [torch.cuda.Event(), torch.cuda.Event()]
                free = [torch.cuda.Event(), torch.cuda.Event()]

                def dbuf(cs, n):
                    for e in free:
                        e.record(cur)
                    with torch.cuda.stream(cs):
                        cs.wait_event(free[0])
                        xd[0].copy_(xh, non_blocking=True); ready[0].record(cs)
                    for it in range(2 + n):
                        if it == 2:
                            torch.cuda.synchronize(); t0 = time.perf_counter()
                        k, kn = it & 1, (it + 1) & 1
                        with torch.cuda.stream(cs):                          # next batch: wait until its buffer's last reader is done
                            cs.wait_event(free[kn])
                            xd[kn].copy_(xh, non_blocking=True); ready[kn].record(cs)
                        cur.wait_event(ready[k])
                        main_w.x = xd[k]
                        main_w.step(False)
                        free[k].record(cur)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) / n
                cands = [torch.cuda.Stream(device=dev) for _ in range(8)]
                trial = [dbuf(c, 3) for c in cands]
                cs = cands[trial.index(min(trial))]
                t = dbuf(cs, n)
                res["double_buffered"] = {"ms_per_step": round(t * 1e3, 3), "images_per_sec": round(B / t, 1),
                                          "copy_stream_trials_ms": [round(v * 1e3, 2) for v in trial]}
                # (c) uint8 HWC frames on the host (what a camera / decoder delivers; 4x fewer bytes over PCIe), /255 + HWC -> CHW on the GPU
                # (exactly the reference's ToTensor arithmetic: uint8 -> float32 / 255); double-buffered as (b).  Timing only: the scenes are
                # re-quantised to 8 bits here
                uh = (keep_x.detach().permute(0, 2, 3, 1) * 255.0).round().clamp_(0, 255).to(torch.uint8).contiguous().cpu().pin_memory()
                ud = [torch.empty(uh.shape, dtype=torch.uint8, device=dev) for _ in range(2)]
                for e in free:
                    e.record(cur)
                with torch.cuda.stream(cs):
                    cs.wait_event(free[0])
                    ud[0].copy_(uh, non_blocking=True); ready[0].record(cs)
                for it in range(2 + n):
                    if it == 2:
                        torch.cuda.synchronize(); t0 = time.perf_counter()
                    k, kn = it & 1, (it + 1) & 1
                    with torch.cuda.stream(cs):
                        cs.wait_event(free[kn])
                        ud[kn].copy_(uh, non_blocking=True); ready[kn].record(cs)
                    cur.wait_event(ready[k])
                    torch.div(ud[k].permute(0, 3, 1, 2), 255.0, out=xd[0])     # uint8 -> float32 / 255, HWC -> CHW, one elementwise kernel
                    free[k].record(cur)
                    main_w.x = xd[0]
                    main_w.step(False)
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) / n
                res["uint8_frames_double_buffered"] = {"batch_bytes_u8": uh.numel(), "ms_per_step": round(t * 1e3, 3), "images_per_sec": round(B / t, 1)}
                main_w.x = keep_x
            return res
        try:
            out["pcie_inclusive"] = pcie_inclusive()
            out["pcie_inclusive"]["note"] = ("host float32 batch -> H2D -> Detector.run_device -> D2H of the boxes; `value` above has the batch "
                                             "resident in HBM (the C-ABI takes device pointers)")
        except Exception as e:                                           # a measurement extra must not take the headline line down
            out["pcie_inclusive"] = {"error": repr(e)[:200]}

    dog = None
    if rank == 0 and world == 1 and not args.no_extras:
        # ---- BASELINE configs[0]: the letterboxed dog image (tests/golden/e2e.npz fixture: uint8 416x416x3), bs=1
        import numpy as np
        gpath = os.path.join(REPO, "tests", "golden", "e2e.npz")
        if os.path.exists(gpath):
            from yolo_v3_amd import Detector
            g = np.load(gpath)
            dog = torch.from_numpy(g["dog_u8"].astype(np.float32) / np.float32(255.0)).permute(2, 0, 1).unsqueeze(0).contiguous()
            net416 = net if args.size == 416 and args.weights == "sw1" else make_net(synth.weight_stream(), 416, dev)
            xd = dog.to(dev)
            lat = {}
            for name, graph in (("eager", False), ("hip_graph", True)):
                d = Detector(net416, 1, 416, 416, 0.5, 0.4, graph=graph)
                with torch.no_grad():
                    for _ in range(5):
                        res = d(xd)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(50):
                        res = d(xd)                                  # full call: kernels + the one D2H sync + list conversion
                    lat[name] = round((time.perf_counter() - t0) / 50 * 1e3, 4)
                nbox = int(res[0].shape[0]) if res else 0
                del d
            out.setdefault("configs", {})["0"] = {"workload": "BASELINE configs[0]: dog-cycle-car.png letterboxed to 416x416 (fixture), bs=1, SW-1 weights, "
                                                              "conf=0.5 nms=0.4, math mode of this run (%s); latency of the whole detect call (kernels + D2H + list conversion), mean of 50" % args.dtype,
                                                  "gpu_ms_per_img": lat, "boxes": nbox}

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle.boxdelta import boxes_delta
        from yolo_v3_amd import detect
        cb, xs, ref_boxes = cpu_baseline(synth.weight_stream() if args.weights != "sw1" else stream, args.conf, args.nms, dog)
        out["cpu_baseline"] = cb
        if "configs" in out and "0" in out["configs"] and "dog_416x416_bs1" in cb["samples"]:
            out["configs"]["0"]["cpu_ms_per_img"] = cb["samples"]["dog_416x416_bs1"]["ms_per_img"]
        # NMS boxes delta vs ref ON THE HEADLINE BATCH ITSELF: the timed Detector (its lanes, its per-launch kernel choice) on the
        # images it was timed on, against the oracle's boxes for the same images (the first 64 of a larger batch; ~6-10 s of CPU)
        from oracle import oracle_cpu as oc
        nb = min(B, 64)
        sd_run, _ = oc.state_dict_from_stream(stream)
        with torch.no_grad():
            ref_boxes = oc.detect(sd_run, x[:nb].cpu(), 80, args.conf, args.nms)
            got = main_w.det(x)
        got = got[:nb] if got else got
        d = boxes_delta(got, ref_boxes, nb)
        out["boxes_delta"] = {
            "vs": "CPU oracle (reference path restated, oracle/oracle_cpu.py) on the images of the timed batch itself (%d of %d), "
                  "result of the timed Detector (lanes=%d)" % (nb, B, main_w.det.lanes), "images": d["images"],
            "ref_boxes": d["ref_boxes"], "got_boxes": d["got_boxes"], "matched_iou_ge_0.999": d["matched"],
            "unmatched_frac": round(d["unmatched_frac"], 6), "count_equal_images": d["count_equal_images"],
            "class_equal_images": d["class_equal_images"], "max_rel_err_coords": float("%.3g" % d["max_rel_err_coords"]),
            "max_abs_err_conf": float("%.3g" % d["max_abs_err_conf"]), "max_abs_err_score": float("%.3g" % d["max_abs_err_score"]),
            "tolerance": 1e-4}
    if rank == 0:
        full_path = write_full(out, args) if args.full else None
        if args.full_line:
            print(json.dumps(out))                                       # an EARLIER stdout line; the compact line stays the last one
        print(json.dumps(compact_line(out, full_path), separators=(",", ":")))
    if world > 1:
        barrier(dev)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
