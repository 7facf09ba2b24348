"""The plans the benchmark actually times, against the CPU oracle (-m gpu, through the C-ABI).

The kernel FORM of a 3x3 layer (direct implicit GEMM or Winograd F(2x2,3x3)) is chosen per launch from the tile count, the
lane count and the CU count (csrc/conv_select.cpp: yv3_select_planes), so "bs=32 one lane is green" does not imply
"bs=64 two lanes is green".  This file closes that gap:

  * the headline workload of bench.py (416x416 bs=64, the 64 scenes ``scenes(64, 416, 1000)``, default math mode) through
    `Detector` with automatic lanes AND with both lane counts forced, all 64 images vs the oracle, with the plan's forms
    asserted through ``yv3_conv2d_form`` (reference path: test.py:35-36);
  * the same in the arithmetic the benchmark's headline is timed in since round 6 -- exact fp32 (``dtype=F32``): two lanes of 32 with 31
    Winograd F(4x4,3x3) launches each, the plain 1x1 layers on the persistent GEMM with its whole-rounds / rest split -- and the other
    exact-fp32 plans bench.py times: the dense 608x608 bs=8 config, eval mode at the reference's thresholds, one image as a HIP graph
    (every launch of these plans against float64: tests/test_gpu_plan_local.py);
  * the whole network with the Winograd form FORCED on every eligible layer (``net.winograd = "always"``), both
    Winograd-capable math modes, vs the oracle and the reference's golden boxes;
  * BASELINE configs[3] at its full size, functionally: 4 ranks (gloo; they time-share the one GPU), global batch 256,
    ``detect_sharded`` == single-GPU ``detect`` of the same 256 images, bit for bit (utils.py:152: images are independent).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle_cpu as oc
from oracle.boxdelta import boxes_delta
from yolo_v3_amd import synth, detect, Detector, _ffi, arch
from tests.helpers import TOL, assert_close_rel, match_boxes, load_sw1_net, detector_dets

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sw1_sd(sw1_stream):
    return oc.state_dict_from_stream(sw1_stream)[0]


@pytest.fixture(scope="module")
def headline(sw1_sd):
    """bench.py's headline batch (``scenes(64, 416, 1000)`` at rank 0 = ``synth.images(64, 416, 1000)``) and the oracle's
    detections + boxes for all 64 images (~6-10 s of CPU)."""
    x = torch.from_numpy(synth.images(64, 416, 1000))
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    with torch.no_grad():
        ref = torch.cat(oc.yolonet_forward(sw1_sd, x), 1)
    return x, ref, oc.postprocess(ref, 80, 0.5, 0.4)


def _form_counts(plan):
    """{(cin, cout, k, stride, Hout): [launches, of which Winograd (either form), of which F(4x4,3x3)]} of one plan's launch sequence."""
    specs = arch.conv_specs()
    hw = arch.conv_output_hw(plan.H)
    out = {}
    for si, f in plan.forms():
        sp = specs[si]
        key = (sp.cin, sp.cout, sp.k, sp.stride, hw[si][0])
        c = out.setdefault(key, [0, 0, 0])
        c[0] += 1
        c[1] += f != 0
        c[2] += f == 2
    return out


def _num_cu():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return n & ~7 if n >= 8 else 256


def _gemm_split_launches(d, ncu):
    """Kernel launches of a plain exact-fp32 1x1 descriptor by the documented rule: the persistent GEMM takes
    the layer when its tiles (128x128; 256x64 for 64 output channels) fill at least one round of the chip; whole rounds run there, and a
    last partial round of at most half the CUs runs on the small tiles instead -- a second launch."""
    M = d.B * d.H * d.W
    bm, bn = (128, 128) if d.cout % 128 == 0 else (256, 64)
    ntn, mt = d.cout // bn, -(-M // bm)
    tiles = mt * ntn
    if tiles < ncu:
        return 1
    rounds, rest = tiles // ncu, tiles % ncu
    here = rounds * ncu // ntn if (rest > 0 and 2 * rest <= ncu) else mt
    return 2 if here * bm < M else 1


ONE_LANE_F4 = 31           # F(4x4,3x3) launches of the one-lane exact-fp32 plan of 64 images on 256 CUs: every eligible layer, as with two lanes (first read on the GPU, then pinned)


def _assert_f32_plan(plan, lanes):
    """The exact-fp32 plan the benchmark times, through ``plan.forms()`` / ``plan.launches()``.  Returns (F(4x4) launches, 1x1 launches split
    between GEMM and tiles, per-shape table)."""
    specs = arch.conv_specs()
    forms, nl = plan.forms(), plan.launches()
    ncu = _num_cu()
    table, n_f4, n_split = {}, 0, 0
    for j, ((si, f), n) in enumerate(zip(forms, nl), plan.first_desc):
        sp, d = specs[si], plan.descs[j]
        key = "%d->%d k%d s%d @%dx%d" % (sp.cin, sp.cout, sp.k, sp.stride, d.H, d.W)
        row = table.setdefault(key, {"launches": 0, "F(4x4)": 0, "kernels": []})
        row["launches"] += 1
        row["kernels"].append(n)
        assert f != 1, "an F(2x2,3x3) launch in the exact-fp32 plan: %s" % key
        if f == 2:
            assert sp.k == 3 and sp.stride == 1 and sp.cin >= 64, key
            assert n == 2, key
            row["F(4x4)"] += 1
            n_f4 += 1
        elif sp.k == 1 and sp.bn and not d.residual and not d.cin_up:
            want = _gemm_split_launches(d, ncu)
            assert n == want and n in (1, 2), "plain 1x1 %s: yv3_conv2d_launches %d, the rest rule gives %d on %d CUs" % (key, n, want, ncu)
            n_split += n == 2
        else:
            assert n == 1, key
    if lanes == 2:
        assert plan.B == 32 and n_f4 == 31, table            # README, BENCH_r06: every stride-1 3x3 layer with cin >= 64
    elif ncu == 256 and ONE_LANE_F4 is not None:
        assert plan.B == 64 and n_f4 == ONE_LANE_F4, table
    return n_f4, n_split, table


@pytest.mark.parametrize("lanes,dtype", [(None, None), (2, None), (1, None), (None, _ffi.F32), (2, _ffi.F32), (1, _ffi.F32)],
                         ids=["None", "2", "1", "None-F32", "2-F32", "1-F32"])
def test_headline_plan_vs_oracle(sw1_stream, headline, lanes, dtype):
    """bench.py's timed step, as bench.py builds it (`Workload`: ``Detector(net, 64, 416, 416, 0.5, 0.4, lanes=None)``), on
    bench.py's 64 scenes: every detection value of all 64 images within 1e-4 * max(1,|ref|) of the oracle, final boxes
    set-wise (class + IOU >= 0.999; random scenes are not margin-selected) with matched boxes within 1e-4 and <= 0.2 %
    unmatched (measured in rounds 3-4: 0 of 5102).  The plan is asserted, not assumed: with two lanes of 32 images every 256->512 @26x26 and 512->1024 @13x13
    layer (18 launches per lane) must take the Winograd form; with one lane of 64 the seven 13x13 layers.  lanes=None is
    the automatic choice the benchmark runs (two lanes at this batch size wherever a concurrent stream pair exists).

    ``dtype=F32`` -- the arithmetic of the benchmark's headline since round 6 -- (``_assert_f32_plan``): no F(2x2) launch; every F(4x4,3x3)
    launch is a 3x3 stride-1 layer with cin >= 64 and two kernels; two lanes: 32 images and 31 F(4x4) launches per lane; one lane of 64:
    ONE_LANE_F4; every plain 1x1 layer reports the kernel count of the GEMM's rest rule (1, or 2 = whole rounds on the GEMM + the rest on
    tiles), every other launch one kernel."""
    x, ref, want = headline
    net = load_sw1_net(sw1_stream).cuda()
    det = Detector(net, 64, 416, 416, 0.5, 0.4, lanes=lanes, dtype=dtype)
    if lanes is not None:
        assert det.lanes == lanes
    with torch.no_grad():
        res = det(x.cuda())
    forms = [_form_counts(p) for p in det.lane_plans]
    if dtype == _ffi.F32:
        for i, p in enumerate(det.lane_plans):
            n_f4, n_split, table = _assert_f32_plan(p, det.lanes)
            print("headline exact fp32, lanes=%s -> %d, lane %d (B=%d): %d F(4x4,3x3) launches, %d plain 1x1 launches split GEMM + tiles"
                  % (lanes, det.lanes, i, p.B, n_f4, n_split))
            for key, row in table.items():
                print("    %-28s launches %2d  F(4x4) %2d  kernels per launch %s" % (key, row["launches"], row["F(4x4)"], sorted(set(row["kernels"]))))
    else:
        c26, c13 = (256, 512, 3, 1, 26), (512, 1024, 3, 1, 13)
        for fc in forms:
            assert fc[c26][0] == 11 and fc[c13][0] == 7
            if det.lanes == 2:
                assert det.lane_plans[0].B == 32 and fc[c26][1] == 11 and fc[c13][1] == 7, fc
            else:
                assert fc[c26][1] == 0 and fc[c13][1] == 7, fc
            assert sum(v[1] for k, v in fc.items() if k not in (c26, c13)) == 0
    err = assert_close_rel(det.dets.cpu(), ref, TOL, "headline detections (lanes=%s)" % det.lanes)
    d = boxes_delta(res, want, 64)
    print("headline plan lanes=%s -> %d: winograd launches per lane %s; max det err %.3g; boxes %s"
          % (lanes, det.lanes, [sum(v[1] for v in fc.values()) for fc in forms], err, d))
    assert d["ref_boxes"] > 600
    assert d["max_rel_err_coords"] <= TOL and d["max_abs_err_conf"] <= TOL and d["max_abs_err_score"] <= TOL
    print("headline lanes=%s: unmatched_frac %.5f (bound 0.002)" % (lanes, d["unmatched_frac"]))
    assert d["unmatched_frac"] <= 0.002, d
    # decisions on IDENTICAL detections (the detector's own) are the oracle's, bit for bit
    exact = oc.postprocess(det.dets.cpu(), 80, 0.5, 0.4)
    assert len(res) == len(exact)
    for a, b in zip(res, exact):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a, b)


def test_dense_config_exact_fp32_vs_oracle():
    """tests/test_gpu_configs.py::test_config5_dense_full_network_vs_oracle in the arithmetic bench.py times the config in
    (``net.math_mode = F32``): 608x608 bs=8 on SW-dense, detections within 1e-4, >= 5000 candidates per image, boxes set-wise with <= 1 %
    unmatched and matched boxes within 1e-4, decisions on the detector's own detections bit-equal to the oracle's."""
    stream = synth.dense_weight_stream()
    net = load_sw1_net(stream, 608).cuda()
    net.math_mode = _ffi.F32
    sd, _ = oc.state_dict_from_stream(stream)
    x = torch.from_numpy(synth.images(8, 608, 4))
    with torch.no_grad():
        ref = torch.cat(oc.yolonet_forward(sd, x), 1)
        got = net.forward_cat(x.cuda()).cpu()
    assert net.engine().dtype == _ffi.F32
    assert_close_rel(got, ref, TOL, "dense config, exact fp32: detections")
    ncand = ((got[..., 5:] * got[..., 4:5]).amax(-1) > 0.5).sum(1)
    assert int(ncand.min()) >= 5000, ncand.tolist()
    res = detect(net, x.cuda(), 80, 0.5, 0.4)
    assert detector_dets(net).dtype == torch.float32 and list(net._detectors.values())[-1].engine.dtype == _ffi.F32
    exact = oc.postprocess(detector_dets(net).cpu(), 80, 0.5, 0.4)
    assert len(res) == len(exact) == 8
    for a, b in zip(res, exact):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a, b)
    d = boxes_delta(res, oc.postprocess(ref, 80, 0.5, 0.4), 8)
    print("dense config, exact fp32: candidates/img %s; boxes %s" % (ncand.tolist(), d))
    assert d["ref_boxes"] > 8 * 2000
    assert d["max_rel_err_coords"] <= TOL and d["max_abs_err_score"] <= TOL
    print("dense config, exact fp32: unmatched_frac %.5f (bound 0.01)" % d["unmatched_frac"])
    assert d["unmatched_frac"] <= 0.01, d


def test_eval_mode_exact_fp32_at_reference_thresholds(golden_dir):
    """tests/test_gpu_configs.py::test_eval_mode_at_reference_thresholds' case as bench.py times it: ``Detector(..., 0.005, 0.45,
    is_eval=True, max_cand=8192, dtype=F32)`` on SW-eval: detections within 1e-4 of the reference's own (tests/golden/e2e_eval.npz),
    decisions on the detector's own detections bit-equal to the oracle's, boxes vs the REFERENCE's set-wise with <= 0.2 % unmatched."""
    g = np.load(os.path.join(golden_dir, "e2e_eval.npz"))
    B, size, seed = [int(v) for v in g["in_cfg"]]
    net = load_sw1_net(synth.eval_weight_stream(), size).cuda()
    x = torch.from_numpy(synth.images(B, size, seed))
    det = Detector(net, B, size, size, 0.005, 0.45, is_eval=True, max_cand=8192, dtype=_ffi.F32)
    with torch.no_grad():
        res = det(x.cuda())
    assert det.engine.dtype == _ffi.F32 and not any(f == 1 for p in det.lane_plans for _, f in p.forms())
    assert_close_rel(det.dets[:, g["rows"]].cpu(), g["dets_rows"], TOL, "SW-eval detections, exact fp32")
    exact = oc.postprocess(det.dets.cpu(), 80, 0.005, 0.45, True, True)
    assert len(res) == len(exact) == B
    for a, b in zip(res, exact):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a, b)
    d = boxes_delta(res, [torch.from_numpy(g["boxes%d" % i]) for i in range(B)], B)
    print("eval mode 0.005/0.45, exact fp32, vs reference:", d)
    assert d["ref_boxes"] > 1000 and d["unmatched_frac"] <= 0.002
    assert d["max_rel_err_coords"] <= TOL and d["max_abs_err_score"] <= TOL


def test_one_image_graph_replay_exact_fp32_equals_eager(sw1_stream):
    """bench.py's one-image HIP-graph config in exact fp32: ``Detector(net, 1, 416, 416, 0.5, 0.4, dtype=F32, graph=True)`` called three
    times equals the eager detector bit for bit -- boxes and the detections tensor.  (One lane: a captured graph without parallel
    branches.  At bs=1 every F(4x4) launch runs the even schedule, whose hand-over flags must be left clean for the next replay.)"""
    net = load_sw1_net(sw1_stream).cuda()
    x = torch.from_numpy(synth.images(1, 416, 1000)).cuda()
    eager = Detector(net, 1, 416, 416, 0.5, 0.4, dtype=_ffi.F32, lanes=1)
    with torch.no_grad():
        want = eager(x)
    want_dets = eager.dets.clone()
    assert sum(f == 2 for _, f in eager.plan.forms()) > 0
    gdet = Detector(net, 1, 416, 416, 0.5, 0.4, dtype=_ffi.F32, graph=True, lanes=1)
    assert gdet.lanes == 1
    for i in range(3):
        gdet.dets.fill_(float("nan"))
        with torch.no_grad():
            got = gdet(x)
        assert gdet._graph is not None
        assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want)), "replay %d" % i
        assert torch.equal(gdet.dets, want_dets), "replay %d: detections differ from the eager run" % i


@pytest.mark.parametrize("B,size,sk", [(4, 416, True), (9, 416, True), (10, 416, False), (4, 608, True), (5, 608, False)])
def test_small_batch_default_plan_vs_oracle(sw1_stream, sw1_sd, headline, B, size, sk):
    """The DEFAULT plan of small batches: up to engine.SK_AUTO_CELLS cells of 32x32 pixels (9 images of 416x416, 4 of 608x608) the
    fp16-plane kernels run the persistent stream-K schedule (a split tile is summed head + tail: within tolerance, not bitwise, of
    the one-tile-per-workgroup schedule) -- asserted on the plan, and every detection value of every image compared with the oracle
    (1e-4 * max(1,|ref|)), final boxes set-wise as in test_headline_plan_vs_oracle."""
    x = headline[0][:B] if size == 416 else torch.from_numpy(synth.images(B, size, 1000 + B))
    net = load_sw1_net(sw1_stream).cuda()
    det = Detector(net, B, size, size, 0.5, 0.4)
    with torch.no_grad():
        res = det(x.cuda())
        ref = headline[1][:B] if size == 416 else torch.cat(oc.yolonet_forward(sw1_sd, x), 1)
    assert det.lanes == 1 and (det.plan.workspace is not None) == sk
    err = assert_close_rel(det.dets.cpu(), ref, TOL, "small-batch default plan B=%d %d" % (B, size))
    d = boxes_delta(res, oc.postprocess(ref, 80, 0.5, 0.4), B)
    print("B=%d %dx%d stream-K %s: max det err %.3g; boxes %s" % (B, size, size, sk, err, d))
    print("B=%d %d: unmatched_frac %.5f (bound 0.005)" % (B, size, d["unmatched_frac"]))
    assert d["max_rel_err_coords"] <= TOL and d["max_abs_err_conf"] <= TOL and d["unmatched_frac"] <= 0.005, d


@pytest.mark.parametrize("mode,n_wino,f4", [(_ffi.F32H2, 18, False), (_ffi.F32, 31, False), (_ffi.F32, 31, True)])
def test_whole_net_forced_winograd_vs_oracle(sw1_stream, sw1_sd, golden_dir, mode, n_wino, f4):
    """``net.winograd = "always"`` (YV3_OPT_WINO_ALWAYS on every descriptor): ALL eligible layers -- 18 in the fp16-plane mode
    (cin >= 256), 31 in the exact-fp32 mode (cin >= 64) -- in the Winograd form at a batch size whose tile counts would
    otherwise select the direct kernels for most of them; 32 images (BASELINE configs[1]'s batch) vs the oracle, plus the
    reference's own golden boxes for the dog image.  Exact-fp32 mode: once with every eligible layer in F(2x2,3x3)
    (``net.winograd4 = False``) and once with every one in F(4x4,3x3) (round 6, csrc/conv_wino4_f32.hip; 13x13, 26x26 pictures hang
    over the 4x4 tile grid)."""
    net = load_sw1_net(sw1_stream).cuda()
    net.winograd = "always"
    net.winograd4 = f4
    net.math_mode = mode
    x = torch.from_numpy(synth.images(32, 416, 1))
    with torch.no_grad():
        ref = torch.cat(oc.yolonet_forward(sw1_sd, x), 1)
        got = net.forward_cat(x.cuda()).cpu()
    plan = net.engine().plan(32, 416, 416)
    fc = _form_counts(plan)
    assert sum(v[1] for v in fc.values()) == n_wino, fc
    assert sum(v[2] for v in fc.values()) == (n_wino if f4 else 0), fc
    assert all(v[1] in (0, v[0]) for v in fc.values())
    err = assert_close_rel(got, ref, TOL, "forced-Winograd detections mode %d" % mode)
    want = oc.postprocess(ref, 80, 0.5, 0.4)
    res = detect(net, x.cuda(), 80, 0.5, 0.4)
    d = boxes_delta(res, want, 32)
    print("forced Winograd mode %d (F(4x4) %s): %d Winograd launches, max det err %.3g; boxes %s" % (mode, f4, n_wino, err, d))
    print("forced Winograd mode %d: unmatched_frac %.5f (bound 0.002)" % (mode, d["unmatched_frac"]))
    assert d["ref_boxes"] > 300 and d["unmatched_frac"] <= 0.002, d
    assert d["max_rel_err_coords"] <= TOL and d["max_abs_err_conf"] <= TOL and d["max_abs_err_score"] <= TOL
    # the reference's own output for the dog image (tests/golden/e2e.npz)
    g = np.load(os.path.join(golden_dir, "e2e.npz"))
    dog = torch.from_numpy(g["dog_u8"].astype(np.float32) / np.float32(255.0)).permute(2, 0, 1).unsqueeze(0).contiguous().cuda()
    with torch.no_grad():
        dets = net.forward_cat(dog)
    assert sum(f != 0 for _, f in net.engine().plan(1, 416, 416).forms()) == n_wino
    e_dog = assert_close_rel(dets[:, g["dog416_rows"]].cpu(), g["dog416_dets_rows"], TOL, "dog image, forced Winograd")
    fused = detect(net, dog, 80, 0.5, 0.4)
    assert len(fused) == int(g["dog416_nres"][0])
    worst = max(match_boxes(f, g["dog416_boxes%d" % i], TOL) for i, f in enumerate(fused))
    print("forced Winograd mode %d, dog image vs the reference's golden: det err %.3g, box err %.3g" % (mode, e_dog, worst))


def test_deterministic_switch_is_bitwise_across_batch_sizes_and_lanes(sw1_stream):
    """``net.deterministic = True``: ONE switch that restores "same image -> same bits" at every batch size, batch position and
    lane request (direct one-tile-per-workgroup kernels, no stream-K, a single lane)."""
    net = load_sw1_net(sw1_stream).cuda()
    net.deterministic = True
    x = torch.from_numpy(synth.images(24, 416, 77)).cuda()
    with torch.no_grad():
        full = net.forward_cat(x).clone()
        one = net.forward_cat(x[5:6]).clone()            # B = 1: stream-K would be automatic without the switch
        part = net.forward_cat(x[16:24]).clone()
    assert torch.equal(full[5:6], one) and torch.equal(full[16:24], part)
    det = Detector(net, 24, 416, 416, lanes=2)             # a requested second lane is declined
    assert det.lanes == 1
    assert all(f == 0 for _, f in det.plan.forms())
    res = det(x)
    res1 = detect(net, x[5:6])
    assert torch.equal(res[5], res1[0]) if res1 else res[5].numel() == 0


def test_config4_full_size_4_ranks_equals_single_gpu():
    """BASELINE configs[3] ("416x416 bs=256 sharded data-parallel across 8 GPUs, RCCL box gather") at its full size, functionally:
    tests/dist_config4_worker.py runs as 4 ranks that time-share this box's one GPU (gloo carries the gather: RCCL wants one GPU
    per rank), each taking its contiguous 64-image shard of the SAME 256 scenes through ``detect_sharded``; rank 0 then runs the
    single-GPU ``detect`` on all 256 images and compares: same list, same shapes, same bits (``net.deterministic = True`` on both
    sides -- with the per-launch kernel choice the 64-image and the 256-image plans may differ in the last bits).  Four ranks, not
    the config's eight: with this test's own process that keeps at most 5 processes on the GPU at once (a shared GPU admits 6); the
    8-way split itself (uneven shards, ranks without images) is covered on CPU by tests/test_dist_gloo.py."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["YV3_DIST_BACKEND"] = "gloo"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "tests", "dist_config4_worker.py")]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print("config 4, 4 ranks on one GPU:", out)
    assert out["world"] == 4 and out["images"] == 256 and out["shard"] == 64 and out["collectives_per_call"] == 1
    assert out["bitwise_equal_images"] == 256 and out["boxes"] > 2000 and out["default_mode_unmatched_frac"] <= 0.002


def test_form_query_mirrors_the_launch_dispatch(sw1_stream, monkeypatch):
    """yv3_conv2d_form must report what yv3_conv2d does.  (a) with the opt-in kw-tap-reuse kernel (YV3_OPT_K3S1, set
    through the measurement environment) the 3x3 stride-1 layers are dispatched to it BEFORE the Winograd rule: form = direct even
    under ``net.winograd = "always"``; (b) a shape the launch rejects (cout not a multiple of 8 for a plane output; a Winograd
    workspace that is too small) gives the same negative code from the query and from the launch."""
    import ctypes
    monkeypatch.setenv("YV3_MEASURE", "1")
    monkeypatch.setenv("YV3_K3S1", "1")
    net = load_sw1_net(sw1_stream).cuda()
    net.winograd = "always"
    net.engine().ensure_packed()
    plan = net.engine().plan(4, 416, 416)
    assert sum(f != 0 for _, f in plan.forms()) == 0
    monkeypatch.delenv("YV3_K3S1")
    net2 = load_sw1_net(sw1_stream).cuda()
    net2.winograd = "always"
    net2.engine().ensure_packed()
    plan2 = net2.engine().plan(4, 416, 416)
    forms = plan2.forms()
    assert sum(f != 0 for _, f in forms) == 18
    lib = _ffi.lib()
    j = plan2.first_desc + [f for _, f in forms].index(1)
    d = type(plan2.descs[j])()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(plan2.descs[j]), ctypes.sizeof(d))
    d.wino_ws_bytes = 16
    assert lib.yv3_conv2d_form(ctypes.byref(d)) == -3 == lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr())     # YV3_EWORKSPACE
    ctypes.memmove(ctypes.byref(d), ctypes.byref(plan2.descs[j]), ctypes.sizeof(d))
    d.cout = d.cout - 4
    assert lib.yv3_conv2d_form(ctypes.byref(d)) == -2 == lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr())     # YV3_ESHAPE
    torch.cuda.synchronize()


def test_stray_tuning_environment_does_not_change_results(sw1_stream, monkeypatch):
    """with YV3_TUNE=0,0,0,7 (the IO ablations: no stores, no residual loads, no decode) and friends in the
    environment -- but no YV3_MEASURE=1 -- detect() returns the same bits as without them: the host side does not read them and
    the shipped library has the branches compiled out."""
    x = torch.from_numpy(synth.images(4, 416, 77)).cuda()
    net = load_sw1_net(sw1_stream).cuda()
    with torch.no_grad():
        want = detect(net, x, 80, 0.5, 0.4)
        dets = net.forward_cat(x).clone()
    monkeypatch.delenv("YV3_MEASURE", raising=False)
    for k, v in (("YV3_TUNE", "0,0,0,7"), ("YV3_TILE", "3"), ("YV3_NO_PP", "1"), ("YV3_WINO_ALWAYS", "1"), ("YV3_NO_FUSED_DECODE", "1")):
        monkeypatch.setenv(k, v)
    net2 = load_sw1_net(sw1_stream).cuda()
    with torch.no_grad():
        got = detect(net2, x, 80, 0.5, 0.4)
        dets2 = net2.forward_cat(x)
    assert torch.equal(dets, dets2)
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    # ... and even a descriptor that carries tune[3] = 7 runs the full epilogue in the shipped library
    plan = net2.engine().plan(4, 416, 416)
    for j in range(plan.n_desc):
        plan.descs[j].tune[3] = 7
    with torch.no_grad():
        dets3 = net2.forward_cat(x)
    assert torch.equal(dets, dets3)


def test_bench_dump_outputs_are_the_last_timed_step(sw1_sd, tmp_path):
    """``bench.py --dump-outputs DIR``: the result line reports exactly ``--steps`` timed steps and their ``ms_per_step``; the files hold
    what the last of them computed on bench.py's seeded scenes (``scenes(2, 416, 1000)`` = ``synth.images(2, 416, 1000)``): the dumped
    sample of the decoded detections within 1e-4 * max(1,|ref|) of the oracle's same rows, the final boxes set-wise as in
    test_small_batch_default_plan_vs_oracle with every row past an image's kept count zero; float32 / float64 only, <= 64 MB."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--batch", "2", "--steps", "3", "--warmup", "1", "--no-extras",
                        "--no-cpu-baseline", "--no-live-traffic", "--dump-outputs", d], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    files = {n[:-len(".npy")]: np.load(os.path.join(d, n)) for n in os.listdir(d)}
    assert set(files) == {"boxes", "counts", "detections_sample", "detection_rows"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 * 10 ** 6
    x = torch.from_numpy(synth.images(2, 416, 1000))
    with torch.no_grad():
        ref = torch.cat(oc.yolonet_forward(sw1_sd, x), 1)
    rows = torch.from_numpy(files["detection_rows"].astype(np.int64))
    assert files["detections_sample"].shape == (2, rows.numel(), ref.shape[2])
    err = assert_close_rel(torch.from_numpy(files["detections_sample"]), ref[:, rows], TOL, "dumped detections")
    kept = files["counts"][:, 1].astype(np.int64)
    assert files["counts"].shape == (2, 2) and (files["counts"][:, 0] >= kept).all()
    assert all(not files["boxes"][i, k:].any() for i, k in enumerate(kept))
    dl = boxes_delta([files["boxes"][i, :k] for i, k in enumerate(kept)], oc.postprocess(ref, 80, 0.5, 0.4), 2)
    print("bench --dump-outputs: %d sampled rows, max det err %.3g; boxes %s" % (rows.numel(), err, dl))
    assert dl["ref_boxes"] > 20 and dl["max_rel_err_coords"] <= TOL and dl["max_abs_err_conf"] <= TOL and dl["unmatched_frac"] <= 0.005, dl


def test_bench_plain_run_is_the_headline_alone():
    """``bench.py`` without ``--full`` on a two-lane step: one result line with the headline fields; its only roofline figure is the
    rate of the timed two-lane section (the one-lane pass takes a run of its own), and none of the --full objects is there (other
    modes, configs, PCIe passes, cpu_baseline, boxes_delta, the side file)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--batch", "4", "--lanes", "2", "--steps", "2", "--warmup", "1"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "images/sec"
    assert out["higher_is_better"] is True and out["dtype"].startswith("f32 (exact fp32") and out["config"]["lanes"] == 2
    assert set(out["roofline"]) == {"two_lanes"} and out["roofline"]["two_lanes"]["achieved"] > 0
    assert not {"stages_ms_one_lane", "cpu_baseline", "boxes_delta", "exact_f32", "f32h2", "f32x3", "bf16", "configs", "pcie_inclusive",
                "full"} & set(out), sorted(out)
