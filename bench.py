#!/usr/bin/env python3
"""bench.py — throughput of the 3D detection / PRM hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload detect|backbone|prm|prm-nuclei|volume] [--stress-rois]
                    [--dump-outputs DIR] [--full [--no-subrecords] [--no-cpu-baseline] [--interleaved] [--pipelined]]

Default workload = BASELINE.json configs[2]: the full detection-mode pipeline of tools/infer_simple.py:249-265 /
lib/core/test.py:54-177 on a batch of 4 synthetic 1x128x128x128 volumes per rank - at every N (weak scaling; `--vols-per-rank 8`
at N = 8 is configs[4]'s 64 volumes, which the N > 1 line also carries as `configs4_shape`).  One "step" = every volume of a batch through
    H2D of the raw uint16 volumes -> norm1 (blob.py:179-184, on device) -> dsn_body -> RPN -> proposals (on device) -> RoIAlign3D ->
    2-MLP head -> decode/clip -> per-class NMS + cap -> cross-tile NMS (core/test.py:159) -> the path's ONE exchange (a single
    all_gather of the padded detections [vols, 301, 7], m3d.shard; a no-op at N = 1) -> D2H of the gathered detections.
THREE distinct batches rotate through the loop (12 different volumes at N = 1: different RoI counts, different branches, nothing of the
input resident in a cache from the step before).
`value` (voxels/s, whole job) is SURVEY 8d's definition: host to host, the raw volumes in pinned host memory when the clock starts, the
detections on the host when it stops (uploads on a copy stream, double-buffered).
A plain run (detect / backbone) does only that: set-up, W warm-up steps, the K timed steps, `--dump-outputs DIR` if given, and the
compact line with the contract's keys.  Everything below is measured with `--full` only (also the full record, see emit()).
`--dump-outputs DIR` writes what the timed path returned in its last timed step as float32 .npy files: `detections.npy`, the gathered
packed detections [N, volumes per rank, 301, 7] that reach the host (m3d.shard layout: a row is one detection's box + score, the
trailer row holds the count), or `feat.npy` for --workload backbone.  Inputs and weights are seeded: the same arguments give the same inputs.
`resident` on the `--full` line is the same loop with the raw volumes already in HBM (the definition of rounds 1-3); `sustained`
repeats that one for at least two seconds.
`roofline` is the metric's named quantity, the 3D-convolution family (dsn_body + RPN convs): `frac` = fp32 MFMA FLOPs ISSUED by all its
launches over their summed live duration (HIP events on the launch stream inside the timed region) against the 157.3 TF peak - the
hardware fraction; `frac_algorithmic` = the direct-convolution count 2*Cin*Cout*k^3 per voxel over the same time against the same peak
(> 1 is possible and is NOT a hardware fraction: Winograd issues 1/3 of those multiplies).  `rooflines` has one entry per layer + fc1.
`cpu_baseline` is the oracle's restatement of the same per-volume pipeline (torch-CPU convs + oracle C ops) on a bounded sample.

Sub-records of the default N = 1 `--full` line (each with ms_per_step, roofline incl. PMC traffic, cpu_baseline; `--no-subrecords` skips them):
  configs1_backbone   BASELINE configs[1]: dsn_body forward alone on ONE 1x128^3 volume
  stress_rois         the default step with the RPN NMS off: RPN_POST_NMS_TOP_N = 1000 RoIs per volume reach the box head
  configs3_prm_soma   BASELINE configs[3]: PRM_ON soma tile 1x64x160x160 -> peak back-propagation -> 2D-Otsu -> instance labels
  prm_nuclei_tile     the same for the nuclei net's 1x64x200x200 tile (the reference's other shipped YAML)
  volume_pipeline     tools/infer_simple.py:176-247 for whole volumes (59x350x350 nuclei, 96x256x256 soma): host array -> per-peak LZW
                      TIFFs + dets.npy on disk, pipelined (m3d.infer.infer_prm)

N > 1: `python bench.py --gpus N` starts N fresh child processes itself (one per GPU, RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* in
their environment, created before this process touches the GPU) unless a launcher (torch.distributed.run) already did.  The N > 1
`--full` line also carries `without_exchange`, `single_gpu_same_batch` (rank 0's batch timed while the other ranks idle) and `exchange`
(the all_gather alone, microseconds, ranks, backend).  Sub-records are an N = 1 matter and are skipped.
`--dry --backend gloo` runs the same launcher + exchange with a stub step on CPU (tests/test_host_logic.py).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))

VOL = 128
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz, no xf32 on gfx950
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: ~2.5 PF dense bf16 MFMA = 16 x the fp32-input MFMA rate (nominal clock; random data holds less)
HBM_PEAK_GBS = 8000.0
WINO_WORK = {0: 1.0, 1: 2.0 / 3.0, 2: 4.0 / 9.0}   # fraction of the algorithmic multiply-adds issued as MFMA work
METRIC = "voxels/sec end-to-end infer_simple (128^3 vol); 3D-conv TFLOPS vs roofline"


# ------------------------------------------------------------------------------------------------ launcher (N > 1)
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(args, argv):
    """Start args.gpus child ranks of this script.  The parent never initialises the GPU (importing torch does not) and
    never exec()s; it waits for the children and returns the worst exit code.  Rank 0's JSON line goes to our stdout."""
    port = int(os.environ.get("MASTER_PORT", "0")) or free_port()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    # wait for all; if one rank dies the others would sit in a collective for ever: stop them (exact PIDs) and report its code
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                for q in live:
                    q.terminate()
        time.sleep(0.2)
    return rc


# ------------------------------------------------------------------------------------------------ helpers
def host_cores():
    """Cores this process may really use: the cgroup CPU quota when there is one (the GPU box shows 256 logical CPUs but
    grants a 16-core share per GPU), else the affinity mask."""
    if "M3D_CPU_THREADS" in os.environ:
        return int(os.environ["M3D_CPU_THREADS"])
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(p))))
    except Exception:
        pass
    return n


def conv_flops(cin, cout, k, vox):
    return 2.0 * cin * cout * k ** 3 * vox


def backbone_flops(size):
    v = size ** 3
    L = [(1, 32, 5, v), (32, 64, 3, v // 8), (64, 64, 3, v // 8), (64, 128, 3, v // 64), (128, 128, 3, v // 64),
         (128, 256, 3, v // 512), (256, 256, 3, v // 512)]
    return sum(conv_flops(*l) for l in L)


def pmc_traffic(symbol_prefix, which="largest", grid_div=None):
    """HBM-side bytes per launch of a kernel from the separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes
    (tools/pmc_probe.py -> tools/pmc_traffic.py -> profiles/rNN_pmc_traffic.json; the counters cannot be collected from inside
    this process, so this is the committed measurement of the same command, newest round first).  A kernel that was launched with
    several grids (batch of 4 / one volume) has one entry per grid: `which` picks the largest or the smallest."""
    import glob
    if grid_div:
        which = "smallest"
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):
        try:
            d = json.load(open(f))
            k = [e for e in d["kernels"] if e["kernel"].replace(" ", "").startswith(symbol_prefix.replace(" ", ""))]
            if k:
                k.sort(key=lambda e: (e.get("grid", 0), e.get("traffic", 0)))
                e = k[0] if which == "smallest" else k[-1]
                return {"traffic": e["traffic"], "traffic_unit": "bytes/launch (FETCH_SIZE x%.2f gfx950 correction + WRITE_SIZE)" %
                        d["calibration"]["fetch_factor_dword_loads"], "traffic_source": os.path.relpath(f, ROOT), "traffic_grid": e.get("grid")}
        except Exception:
            continue
    return {"traffic": None}


def sync_max_time(dt, dist, device):
    import torch
    if dist is None:
        return dt
    t = torch.tensor([dt], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """--dump-outputs: name -> tensor the timed path returned, written as out_dir/<name>.npy in float32.  An array beyond its share of
    DUMP_MAX_BYTES is replaced by a fixed seeded sample of its flattened elements (in index order), so that runs compare element for element."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_MAX_BYTES // max(1, len(arrays))
    for name, t in arrays.items():
        a = np.ascontiguousarray(t.detach().to("cpu", torch.float32).numpy())
        if a.nbytes > share:
            a = a.ravel()[np.sort(np.random.RandomState(0).choice(a.size, share // 4, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


PROBE_STEPS = 3        # timed steps that carry per-kernel HIP-event spans (the rooflines' live durations); the rest run bare


def timed_loop(step, steps, warmup, dist, sync):
    """The contract's timing: W untimed steps, then exactly K steps between barrier + device synchronize on both sides.
    (gc.collect() + gc.disable() around the timed steps was tried against host hiccups: the 20-step region got 3 % SLOWER, 4.61 against
    4.47 ms per step in four A/B runs - the interpreter's allocator does not like the full collection in front of it - so the
    collector is left alone.)"""
    for _ in range(warmup):
        step()
    sync()
    if dist is not None:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    sync()
    if dist is not None:
        dist.barrier()
    sync()
    return time.perf_counter() - t0


# ------------------------------------------------------------------------------------------------ dry run (CPU, gloo)
def run_dry(args, rank, world, dist):
    """Launcher + exchange rehearsal without a GPU: every rank fabricates its volumes' detections, the ONE all_gather
    of m3d.shard moves them, every rank checks the global list."""
    import torch
    from m3d import shard
    nvol = args.vols_per_rank or 4
    n_items = world * nvol
    cap = 300

    def fake(i):                                   # item i: (i % 7) + 1 detections whose columns all hold i
        return torch.full(((i % 7) + 1, 7), float(i))
    mine = shard.partition(n_items, rank, world)
    assert len(mine) == nvol
    if os.environ.get("M3D_BENCH_TEST_KILL_RANK") == str(rank):       # tests/test_host_logic.py: a rank that dies must not hang the rest
        os._exit(7)

    def step():
        got = shard.all_gather_detections([fake(i) for i in mine], cap, n_items, dist)
        assert len(got) == n_items
        for i, t in enumerate(got):
            assert t.shape == ((i % 7) + 1, 7) and float(t[0, 0]) == float(i), (i, t.shape)
    dt = timed_loop(step, args.steps, args.warmup, dist, lambda: None)
    dt = sync_max_time(dt, dist, "cpu")
    xchg = None
    if dist is not None:                                   # the exchange alone, as the GPU line reports it
        mine_t = [fake(i) for i in mine]
        nx = 10
        dtx = timed_loop(lambda: shard.all_gather_detections(mine_t, cap, n_items, dist), nx, 2, dist, lambda: None)
        xchg = {"us": sync_max_time(dtx, dist, "cpu") / nx * 1e6, "ranks": world, "backend": dist.get_backend(),
                "bytes_per_rank": int(nvol * (cap + 1) * 7 * 4)}
    if rank == 0:
        print(compact_line({"metric": METRIC, "value": 0.0, "unit": "voxels/s", "n_gpus": world, "steps": args.steps,
                            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "dry": True,
                            "config": {"workload": "DRY RUN (no GPU): launcher + one all_gather of [%d,%d,7] per rank, stub detect step"
                                       % (nvol, cap + 1), "volumes_per_step": n_items, "volumes_per_rank": nvol, "backend": args.backend},
                            "exchange": xchg}), flush=True)


# ------------------------------------------------------------------------------------------------ PRM workloads
def cone_limited_gflop_per_peak(stride, in_size=None, strip_zw=True):
    """(algorithmic GFLOP, matrix-pipe milliseconds at peak, issued GFLOP) of one peak's back-propagation when every layer only computes its
    receptive-field window: window side per layer from the top (3 -> 5 -> 7 at the RPN stride, x2 + border after each
    un-pool), 2*Cin*Cout*k^3 per voxel of the n^3 window.  Issued = what the kernels put on the matrix cores: every fp32 product for the
    small windows (their f16x2 form since round 6: 3 f16 products per product); for the strips the voxels the strip really holds (planes:
    min(n, depth of the layer's map) - the depth-clipped strips -, rows n, columns the strip's pitch) x 2 f16 products per multiply-add
    where the strip runs on the f16x2 F(2,3)z kernel (round 6: backward-data convs with >= 64 output channels) or x 1/3 fp32 products
    (F(2x4,3x3): the 64 -> 32 layer); the 5^3 stem occupies 32 fp32 MFMA rows for its 25 (dy, dx) taps.  Pipe time = issued / the peak of
    each launch's operand type (fp32 157.3 TF, f16 2500 TF)."""
    if stride == 8:
        L = [(256, 256, 3, 3, 8), (256, 256, 3, 5, 8), (256, 128, 3, 7, 8), (128, 128, 3, 16, 4), (128, 64, 3, 18, 4), (64, 64, 3, 38, 2),
             (64, 32, 3, 40, 2), (32, 1, 5, 84, 1)]
    else:
        L = [(128, 128, 3, 3, 4), (128, 128, 3, 5, 4), (128, 64, 3, 7, 4), (64, 64, 3, 16, 2), (64, 32, 3, 18, 2), (32, 1, 5, 40, 1)]
    depth = (in_size[0] if in_size else 64)
    alg = sum(2.0 * a * b * k ** 3 * n ** 3 for a, b, k, n, _ in L) / 1e9
    issued = 0.0
    pipe_s = 0.0
    for a, b, k, n, down in L:
        peak = FP32_MFMA_PEAK_TFLOPS
        if k == 5:
            vox, f = n ** 3, 32.0 / 25.0
        elif n >= 16:
            pitch = 4 * ((n + (1 if n % 4 else 0) + 3) // 4) if n % 4 else n + 4      # quad-aligned strip (strip_geom mode 2): 16 -> 20, 18 -> 20, 38 -> 40, 40 -> 44
            vox = min(n, depth // down) * n * pitch
            if strip_zw and b >= 64 and a % 16 == 0:
                f, peak = 2.0, BF16_MFMA_PEAK_TFLOPS
            else:
                f = 1.0 / 3.0
        else:
            vox, f = n ** 3, (3.0 if a % 16 == 0 else 1.0)                          # small-window GEMMs: f16x2 where the forward cout % 16 == 0
            if a % 16 == 0:
                peak = BF16_MFMA_PEAK_TFLOPS
        fl = 2.0 * a * b * k ** 3 * vox * f
        issued += fl
        pipe_s += fl / (peak * 1e12)
    return alg, pipe_s * 1e3, issued / 1e9


def bench_prm(args, rank, world, dist, cpu_budget_s=25.0):
    """configs[3]: PRM_ON soma tile 1x64x160x160 (or the nuclei net's 1x64x200x200 tile): forward (2 convs per layer) + batched peak
    back-propagation + per-detection Otsu binarisation down to instance labels.  Returns the result dict on rank 0."""
    import numpy as np
    import torch
    import m3d
    from m3d.model import DetectorM3D, Probe
    from m3d.prm import PRMEngine
    from m3d.config import Cfg
    from m3d.synth import synth_volume
    from m3d import tiling
    nuclei = args.workload == "prm-nuclei"
    cfg = Cfg.nuclei(score_thresh=0.0) if nuclei else Cfg.soma()
    P = prm_params(cfg, args)
    eng = PRMEngine(DetectorM3D({k: v.cuda() for k, v in P.items()}, cfg), norm_stream=bool(getattr(args, "prm_norm_stream", 1)),
                    backward_streams=int(getattr(args, "prm_backward_streams", 1)), strip_f24_min=int(getattr(args, "prm_f24_min", 16)),
                    fused_prepare=bool(int(getattr(args, "prm_fused_prepare", 1))))
    S, H, W = cfg.in_size
    vol = torch.from_numpy(tiling.norm1(synth_volume(rank, (S, H, W)), np.float32).astype(np.float32)).reshape(1, 1, S, H, W).cuda()
    from m3d import binarize
    raw = torch.from_numpy(synth_volume(rank, (S, H, W)).astype(np.uint16)).cuda()
    mode = "nuclei" if nuclei else "soma"
    npk, nlab = [], []
    last = {"out": None}
    stamps = []
    pr = {"probe": None, "left": 0}
    bstream = torch.cuda.Stream() if int(getattr(args, "prm_binarize_stream", 1)) else None

    from m3d.prm import TilePipeline
    pipe = TilePipeline(eng, dense=False) if int(getattr(args, "prm_pipeline", 0)) else None

    def post(out):
        """a tile's maps -> instance labels (binarization_*.py loop body)"""
        npk.append(0 if out is None else int(out["peaks"].shape[0]))
        last["out"] = out
        if out is None:
            return
        if bstream is not None:                        # on a second stream: beside the next tile's forward (span events on that stream)
            labels, painted, _ = binarize.segment_tile_on(bstream, raw, (out["windows"], out["sums"], out["origins"]), out["dets"],
                                                          span=eng.span("binarize"), mode=mode)
        else:
            with eng.span("binarize"):
                labels, painted = binarize.segment_tile(raw, (out["windows"], out["sums"], out["origins"]), out["dets"], mode=mode)
        nlab.append(painted)

    def step():
        """one tile: PRM forward + box head + peak back-propagation -> uint8 quantisation (from the windows; no dense float maps) -> per-detection crop +
        normalisation -> 2D-Otsu -> largest component (+ hole fill / closing) -> instance labels.  With the tile pipeline a step enqueues tile k's
        forward and FINISHES tile k - 1 (m3d.prm.TilePipeline); `drain` finishes the last tile inside the timed region."""
        stamps.append(time.perf_counter())
        eng.probe = eng.det.probe = pr["probe"] if pr["left"] > 0 else None
        pr["left"] -= 1
        if pipe is None:
            post(eng.prm_tile(vol, dense=False))
        else:
            for _, out in pipe.push(None, vol):
                post(out)

    def drain():
        if pipe is not None:
            for _, out in pipe.flush():
                post(out)
        torch.cuda.synchronize()
    pr["probe"], pr["left"] = Probe(), args.warmup         # throw-away probe on the warm-up steps (event pool)
    for _ in range(args.warmup):
        step()
    drain()
    import gc
    gc.collect()
    gc.freeze()                                            # (see bench_detect: a full collection over ~10^6 objects costs 40-60 ms)
    probe = Probe()
    pr["probe"], pr["left"] = probe, PROBE_STEPS
    dt = timed_loop(step, args.steps, 0, dist, drain)
    dt = sync_max_time(dt, dist, "cuda")
    torch.cuda.synchronize()
    eng.probe = eng.det.probe = None
    step_ms = [(b - a) * 1e3 for a, b in zip(stamps[args.warmup:-1], stamps[args.warmup + 1:])][1:args.steps]      # host-side step starts (the
    # host waits inside every tile, so they follow the GPU); the first one still holds the warm-up's tail
    ph = probe.median_ms()
    probe.spans.clear()
    npeaks = npk[-1] if npk else 0
    # peaks whose RPN sigmoid is saturated are skipped by the engine (their map is exactly 0 / 0, m3d.prm skip_dead_peaks): only the
    # back-propagated ones count as work
    nlive = int((last["out"]["sums"] > 0).sum().item()) if last["out"] is not None else 0
    back_ms = ph.get("backward")
    fwd_ms = (ph.get("forward_response", 0.0) + ph.get("norm_convs", 0.0) + ph.get("norm_convs_late", 0.0)) or None
    otsu_ms = ph.get("binarize")
    # cone-limited work of the back-propagation: receptive-field windows per layer, dgrad with relu(W); algorithmic =
    # 2*Cin*Cout*k^3 per window voxel, issued = what the kernels put on the matrix cores (strips: 4/9 or 1/3 of the products of the voxels
    # the strip holds, every product for the small-window GEMMs, 32/25 for the stem whose 25 (dy, dx) taps occupy 32 MFMA rows)
    cone, pipe_ms, cone_issued = cone_limited_gflop_per_peak(cfg.stride, cfg.in_size, strip_zw=eng.strip_zw)
    dom = "prm_stem_dgrad_mfma_kernel<40, 2, 5>" if nuclei else "prm_stem_dgrad_mfma_kernel<18, 3, 4>"     # the largest backward launch
    roof = None
    if back_ms and nlive:
        frac = nlive * pipe_ms / back_ms
        roof = {"bound": "mfma", "kernel": "peak back-propagation of the tile's %d peaks (%d back-propagated, the rest saturated: map 0 / 0): prm_seed, "
                                           "prm_prepare*, the strip / small-window / stem dgrad kernels, window sums - the backward kernels "
                                           "ONLY (HIP-event span around them)" % (npeaks, nlive),
                "achieved": frac * FP32_MFMA_PEAK_TFLOPS, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": frac,
                "frac_algorithmic": nlive * cone / back_ms / FP32_MFMA_PEAK_TFLOPS,
                "algorithmic_tflops": nlive * cone / back_ms,
                "cone_limited_gflop_per_peak": cone, "issued_gflop_per_peak": cone_issued, "pipe_ms_at_peak_per_peak": pipe_ms, "backward_ms": back_ms,
                "frac_definition": "frac = the window convolutions' matrix-pipe time at peak / backward_ms: per layer, FLOPs issued / the peak of "
                                   "the layer's operand type - fp32 MFMA 157.3 TF for the stem (32 MFMA rows for 25 taps) and the 64 -> 32 strip "
                                   "(F(2x4,3x3): 1/3 of the products), f16 MFMA 2 500 TF for the f16x2 launches (round 6: strips with >= 64 "
                                   "output channels on the F(2,3)z kernel, 2 f16 products per multiply-add of the voxels the strip holds; the "
                                   "3^3 / 5^3 / 7^3 window GEMMs, 3 per multiply-add).  achieved = frac x the fp32 peak (fp32-equivalent "
                                   "TFLOP/s).  frac_algorithmic = the cone-limited direct count (n^3 windows) over the same time / the fp32 "
                                   "peak.  backward_ms is a span on the tile's stream and includes the time the first layers share the chip "
                                   "with the norm convs of the second stream"}
        t = pmc_traffic(dom, which="largest")
        roof["traffic"] = t.get("traffic")
        roof["traffic_what"] = "HBM bytes per launch of the largest backward kernel (%s), PMC: %s" % (dom, t.get("traffic_source"))
    res = {"metric": "voxels/sec end-to-end infer_simple (PRM_ON tile)", "value": world * args.steps * S * H * W / dt,
           "unit": "voxels/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": dt / args.steps * 1e3, "ms_per_step_median": (sorted(step_ms)[len(step_ms) // 2] if step_ms else None),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": ("PRM tile 1x%dx%dx%d %s net: PRM forward + box head + batched peak back-propagation + per-detection 2D-Otsu -> instance labels%s" %
                                  (S, H, W, "nuclei (stride 8, 35 anchors)" if nuclei else "soma (stride 4, 14 anchors)",
                                   "" if nuclei else " [configs[3]]")), "peaks_per_tile": npeaks, "peaks_back_propagated": nlive,
                      "phase_ms": {k: round(v, 4) for k, v in sorted(ph.items(), key=lambda kv: -kv[1])},
                      "phase_note": "; ".join(
                          (["norm_convs is a span on a SECOND stream: it runs beside proposals / box_head and the first layers of backward"] if eng.norm_stream else []) +
                          (["binarize is a span on a THIRD stream: tile k's binarisation runs beside tile k+1's forward (ms_per_step = time of the timed "
                            "steps / steps, every stream drained before the clock stops)"] if bstream is not None else [])) or "all phases on one stream",
                      "prm_forward_ms": fwd_ms, "prm_backward_ms": back_ms, "instances_painted": int(nlab[-1].sum()) if nlab else 0,
                      "step_starts_ms_host": [round((b - a) * 1e3, 2) for a, b in zip(stamps[args.warmup:-1], stamps[args.warmup + 1:])][:args.steps]},
           "roofline": roof,
           "otsu": {"rois": npeaks, "ms": otsu_ms, "rois_per_s": npeaks / otsu_ms * 1e3 if otsu_ms else None,
                    "what": "uint8 quantisation + crop + normalise + 2D-Otsu + largest component%s + painting for the tile's detections" %
                            (" + hole fill + 6-closing" if nuclei else "")}}
    if rank != 0:
        return None
    if not args.no_cpu_baseline and world == 1 and npeaks > 0:
        # CPU baseline leg (the only use of oracle/ here): the oracle's restatement of PeakResponseMapping_3d.forward on the SAME tile,
        # back-propagating a capped number of peaks (a peak costs seconds of dense autograd-equivalent work on the CPU), extrapolated
        # per peak to the tile's peak count; + the per-detection Otsu loop body on the same capped sample
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        ncpu = host_cores()
        torch.set_num_threads(ncpu)
        ocfg = O.Cfg(score_thresh=0.0) if nuclei else O.Cfg.soma()
        xc = vol.cpu()
        c0 = time.perf_counter()
        O.prm_tile(P, ocfg, xc, max_peaks=0)               # forward (2 convs per layer) + proposals + box head + box results
        t_fwd = time.perf_counter() - c0
        cap_peaks = min(2, npeaks)
        c0 = time.perf_counter(); got = O.prm_tile(P, ocfg, xc, max_peaks=cap_peaks); t_peaks = max(time.perf_counter() - c0 - t_fwd, 1e-9)
        more = min(8, npeaks)
        if npeaks > cap_peaks and 2 * t_fwd + (cap_peaks + more) * t_peaks / cap_peaks < cpu_budget_s:     # capped at 8 peaks
            cap_peaks = more
            c0 = time.perf_counter(); got = O.prm_tile(P, ocfg, xc, max_peaks=cap_peaks); t_peaks = max(time.perf_counter() - c0 - t_fwd, 1e-9)
        per_peak = t_peaks / cap_peaks
        # Otsu stage of the capped sample (quantised maps of the back-propagated peaks)
        prms = got[2].numpy()
        qc = np.stack([O.quantize_prm_u8(m_) for m_ in prms])
        bx = binarize.det_boxes_int(np.asarray(got[3])[:cap_peaks], (S, H, W), mode)
        c0 = time.perf_counter()
        O.segment_tile(raw.cpu().numpy(), qc, bx, mode)
        per_roi = (time.perf_counter() - c0) / cap_peaks
        t_tile = t_fwd + nlive * per_peak + npeaks * per_roi        # like for like: the peaks the GPU back-propagated; every detection binarised
        res["cpu_baseline"] = {"value": S * H * W / t_tile, "unit": "voxels/s", "cores": ncpu, "kind": "port",
                               "sample": "the same tile through the oracle's restatement (torch-CPU convs with %d threads, oracle C box ops): forward + box "
                                         "head %.2f s measured; %d of the tile's %d peaks back-propagated (%.2f s per peak) and binarised (%.3f s per "
                                         "detection), extrapolated to the %d peaks the GPU back-propagated and all %d detections" % (ncpu, t_fwd, cap_peaks, npeaks, per_peak, per_roi, nlive, npeaks),
                               "seconds_per_tile_extrapolated": t_tile}
        res["speedup_vs_cpu_baseline"] = res["value"] / res["cpu_baseline"]["value"]
    return res


# ------------------------------------------------------------------------------------------------ whole volumes (PRM mode, to files)
def bench_volume(args, rank, world, dist, datasets=("nuclei", "soma"), reps=2, cpu_budget_s=12.0):
    """tools/infer_simple.py:176-247 for whole volumes: host uint16 array -> norm1 -> pad -> tiles -> PRM -> per-peak uint8 LZW TIFFs +
    dets.npy on disk (m3d.infer.infer_prm: device norm1 in float64, uint8 windows to pinned memory on a copy stream, pages rebuilt and
    encoded by a thread pool).  nuclei: 59x350x350 -> 9 tiles of 64x200x200; soma: 96x256x256 -> 12 tiles of 64x160x160.
    Output goes to a scratch directory (tmpfs when there is one) that is removed afterwards."""
    import shutil
    import tempfile
    import numpy as np
    import torch
    from m3d.model import DetectorM3D
    from m3d.prm import PRMEngine
    from m3d.config import Cfg
    from m3d.synth import synth_volume
    from m3d import infer as minfer, tiling
    out = {}
    base = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    for ds in datasets:
        cfg = Cfg.nuclei(score_thresh=0.0) if ds == "nuclei" else Cfg.soma()
        shape = (59, 350, 350) if ds == "nuclei" else (96, 256, 256)
        P = prm_params(cfg, args)
        eng = PRMEngine(DetectorM3D({k: v.cuda() for k, v in P.items()}, cfg))
        im = synth_volume(100 + rank, shape)
        scratch = tempfile.mkdtemp(prefix="m3d_vol_", dir=base)
        try:
            def run(tag, fn):
                d = os.path.join(scratch, tag)
                t0 = time.perf_counter()
                res_ = fn(eng, im, dataset=ds, out_dir=d, **({"keep_maps": False} if fn is minfer.infer_prm else {}))
                torch.cuda.synchronize()
                dt_ = time.perf_counter() - t0
                nfiles = sum(len(f) for _, _, f in os.walk(d))
                nbytes = sum(os.path.getsize(os.path.join(r_, f)) for r_, _, fs in os.walk(d) for f in fs)
                shutil.rmtree(d, ignore_errors=True)
                return dt_, res_, nfiles, nbytes
            run("warm", minfer.infer_prm)                                  # first launches, pinned pools, thread pool
            import gc
            gc.collect()
            gc.freeze()
            times = []
            for k in range(reps):
                dt_, res_, nfiles, nbytes = run("p%d" % k, minfer.infer_prm)
                times.append(dt_)
            dt_p = min(times)
            dt_s, res_s, nfiles_s, _ = run("serial", minfer.infer_prm_serial)
            # one more (untimed) pipelined pass with HIP-event spans around every tile's back-propagation: the volume's roofline
            from m3d.model import Probe
            vp = Probe()
            eng.probe = vp
            run("probe", minfer.infer_prm)
            eng.probe = None
            back_ms = sum(a_.elapsed_time(b_) for a_, b_ in vp.spans.get("backward", []))
            vp.spans.clear()
            vox = float(np.prod(shape))
            peaks = int(sum(len(r_["dets"]) for r_ in res_))
            # saturated peaks are skipped by the engine (m3d.prm skip_dead_peaks): only the back-propagated ones count as work
            live = int(sum(r_.get("peaks_back_propagated", len(r_["dets"])) for r_ in res_))
            rec = {"value": vox / dt_p, "unit": "voxels/s", "seconds_per_volume": dt_p, "seconds_per_volume_runs": [round(t, 4) for t in times],
                   "volume": "%dx%dx%d uint16 (%s net)" % (shape + (ds,)), "tiles_with_detections": len(res_), "peaks": peaks, "peaks_back_propagated": live,
                   "files_written": nfiles, "bytes_written": nbytes, "writer_threads": minfer.writer_pool().workers,
                   "serial_driver": {"value": vox / dt_s, "seconds_per_volume": dt_s, "files_written": nfiles_s,
                                     "what": "infer_prm_serial: dense uint8 maps copied back and written tile by tile (round 3's driver with the "
                                             "device norm1)"},
                   "what": "host uint16 volume -> per-peak LZW TIFFs + dets.npy in a scratch directory (%s), pipelined; best of %d"
                           % ("tmpfs" if base else "tmp", reps)}
            cone, pipe_ms, cone_issued = cone_limited_gflop_per_peak(cfg.stride, cfg.in_size, strip_zw=eng.strip_zw)
            if back_ms > 0 and live:
                dom = "prm_stem_dgrad_mfma_kernel<40, 2, 5>" if ds == "nuclei" else "prm_stem_dgrad_mfma_kernel<18, 3, 4>"
                rec["roofline"] = {"bound": "mfma", "kernel": "peak back-propagation of the volume's %d peaks (%d back-propagated, the rest saturated: map "
                                                              "0 / 0) over %d tiles (backward kernels only, HIP-event spans of one extra untimed pass)"
                                                              % (peaks, live, len(res_)),
                                   "achieved": live * pipe_ms / back_ms * FP32_MFMA_PEAK_TFLOPS, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                                   "frac": live * pipe_ms / back_ms,
                                   "frac_algorithmic": live * cone / back_ms / FP32_MFMA_PEAK_TFLOPS, "kernel_ms": back_ms,
                                   "share_of_volume_time": back_ms * 1e-3 / dt_p, "traffic": pmc_traffic(dom, which="largest").get("traffic")}
            if rank == 0 and not args.no_cpu_baseline and world == 1:
                # CPU leg: the oracle's PRM tile on ONE tile of this volume with a capped number of peaks, extrapolated to all tiles and
                # peaks, + the reference-style per-page Python TIFF writer on the dense uint8 maps of that sample
                sys.path.insert(0, os.path.join(ROOT, "oracle"))
                import oracle as O
                from m3d import io as mio
                ncpu = host_cores()
                torch.set_num_threads(ncpu)
                ocfg = O.Cfg(score_thresh=0.0) if ds == "nuclei" else O.Cfg.soma()
                patch = cfg.in_size
                vol64 = tiling.norm1(im, np.float64)
                vol64, pad_s = tiling.pad_slices(vol64, patch[0])
                crop = torch.from_numpy(vol64[:patch[0], :patch[1], :patch[2]].astype(np.float32))[None, None]
                c0 = time.perf_counter(); O.prm_tile(P, ocfg, crop, max_peaks=0); t_fwd = time.perf_counter() - c0
                capk = 2
                c0 = time.perf_counter(); got = O.prm_tile(P, ocfg, crop, max_peaks=capk); t_pk = max(time.perf_counter() - c0 - t_fwd, 1e-9) / capk
                t_wr = 0.0
                if got[2] is not None and len(got[2]):
                    c0 = time.perf_counter()
                    q = O.quantize_prm_u8(got[2][0].numpy().copy())
                    mio.write_tiff_stack(os.path.join(scratch, "cpu.tif"), q)
                    t_wr = time.perf_counter() - c0
                ntiles = len(tiling.enumerate_tiles(*tiling.tile_grid(vol64.shape, patch, cfg.crop_ovlp, ds)))
                t_vol = ntiles * t_fwd + live * t_pk + peaks * t_wr
                rec["cpu_baseline"] = {"value": vox / t_vol, "unit": "voxels/s", "cores": ncpu, "kind": "port",
                                       "sample": "one %dx%dx%d tile of the volume through the oracle (forward + box head %.2f s; %d peaks back-propagated, "
                                                 "%.2f s each; one map quantised + written, %.3f s), extrapolated to the volume's %d tiles, the %d peaks "
                                                 "the GPU back-propagated (saturated ones cost the CPU leg nothing either) and %d maps written"
                                                 % (patch + (t_fwd, capk, t_pk, t_wr, ntiles, live, peaks)),
                                       "seconds_per_volume_extrapolated": t_vol}
            out[ds] = rec
        finally:
            shutil.rmtree(scratch, ignore_errors=True)
        del eng
        torch.cuda.empty_cache()
    if rank != 0:
        return None
    lead = out[datasets[0]]
    return {"metric": "voxels/sec end-to-end infer_simple (PRM_ON whole volume, to files)", "value": lead["value"], "unit": "voxels/s",
            "n_gpus": world, "steps": reps, "warmup": 1, "ms_per_step": lead["seconds_per_volume"] * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "whole-volume PRM-mode infer_simple (tools/infer_simple.py:176-247): host array -> tiles -> PRM -> per-peak LZW TIFFs + dets.npy"},
            "roofline": lead.get("roofline"), "volumes": out, "cpu_baseline": lead.get("cpu_baseline")}


# ------------------------------------------------------------------------------------------------ detect / backbone
NB = 3                 # distinct batches rotating through every detect loop (the same step on the same data measures a warm cache)
_params_cache = {}


def prm_params(cfg, args):
    """Parameters of the PRM workloads.  The nuclei net's random init gives RPN class logits of +-40: the sigmoid of every top-ranked
    position is exactly 1.0f, its derivative (1 - y) y exactly 0, and the reference's back-propagation then returns 0 / 0 maps for
    EVERY kept peak of the tile (rounds 1-3 timed that: the kernels' time does not depend on the values, but the binarisation stage and
    the LZW writer saw all-zero maps).  RPN_cls_score's weight and bias are therefore scaled by --prm-rpn-logit-scale (default 0.25:
    logits of +-10 as a trained net has; the ranking of the proposals is the same monotone function of the same logits); 1.0
    reproduces the earlier rounds' workload.  Round 6: the soma net (stride 4) is scaled too - rounds 1-5 left it saturated, a quarter
    of configs[3]'s 128 peaks and most of the soma volume's were dead (and skipped since round 5), which flattered those records."""
    from m3d.synth import unsaturated_rpn
    P = cached_params(stride=cfg.stride, num_anchors=cfg.num_anchors, mlp_dim=cfg.mlp_dim, seed=0)
    a = float(getattr(args, "prm_rpn_logit_scale", 0.25))
    return unsaturated_rpn(P, a) if a != 1.0 else P


def cached_params(**kw):
    """make_params is ~2 s of CPU random numbers for the nuclei net (90 M fc1 weights): the sub-records share them."""
    from m3d.synth import make_params
    key = tuple(sorted(kw.items()))
    if key not in _params_cache:
        _params_cache[key] = make_params(**kw)
    return _params_cache[key]


def conv_family_roofline(det, work, kern_ms, nvol, what_batch):
    """`roofline` of the 3D-convolution family from live HIP-event spans.  Per launch: frac = matrix-core FLOPs ISSUED / time / the peak of
    the launch's operand type (fp32 MFMA 157.3 TF for the fp32 Winograd kernels, f16 MFMA 2 500 TF for the f16x2 kernels of round 6);
    frac_algorithmic = direct-convolution FLOPs / time / the fp32 peak (may exceed 1: Winograd, 16-bit matrix cores).  Family: the launches'
    matrix-pipe time at peak (sum of issued / peak) over their summed duration."""
    roofs = {}
    fam_pipe_s = fam_alg = fam_ms = fam_f16_issued = fam_f32_issued = 0.0
    for name, wk in work.items():
        if name not in kern_ms:
            continue
        ms = kern_ms[name]
        f16 = wk.get("dtype") == "f16"
        peak = BF16_MFMA_PEAK_TFLOPS if f16 else FP32_MFMA_PEAK_TFLOPS
        fam_pipe_s += wk["issued_flop"] / (peak * 1e12); fam_alg += wk["algorithmic_flop"]; fam_ms += ms
        if f16:
            fam_f16_issued += wk["issued_flop"]
        else:
            fam_f32_issued += wk["issued_flop"]
        ach = wk["issued_flop"] / (ms * 1e-3) / 1e12
        alg = wk["algorithmic_flop"] / (ms * 1e-3) / 1e12
        roofs[name] = {"bound": "mfma", "kernel": wk["kernel"], "shape": wk["shape"], "launch": "one launch over %s" % what_batch,
                       "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "operands": "f16" if f16 else "f32",
                       "frac_algorithmic": alg / FP32_MFMA_PEAK_TFLOPS, "kernel_ms": ms,
                       "issued_gflop_per_launch": wk["issued_flop"] / 1e9, "algorithmic_gflop_per_launch": wk["algorithmic_flop"] / 1e9,
                       "algorithmic_tflops": alg}
    fam = None
    if fam_ms > 0:
        frac = fam_pipe_s / (fam_ms * 1e-3)
        alg = fam_alg / (fam_ms * 1e-3) / 1e12
        mixed = fam_f16_issued > 0
        peak = BF16_MFMA_PEAK_TFLOPS if mixed else FP32_MFMA_PEAK_TFLOPS
        fam = {"bound": "mfma",
               "kernel": "3D-convolution family: dsn_body conv1a..conv4b (+BN+ReLU+MaxPool fused)%s, %d launches over %s"
                         % (" and the RPN convs" if "rpn" in kern_ms else "", len([n for n in work if n in kern_ms]), what_batch),
               "achieved": frac * peak, "peak": peak, "unit": "TFLOP/s", "frac": frac,
               "frac_algorithmic": alg / FP32_MFMA_PEAK_TFLOPS, "algorithmic_tflops": alg, "kernel_ms": fam_ms,
               "issued_gflop_per_step": (fam_f16_issued + fam_f32_issued) / 1e9, "issued_f16_gflop_per_step": fam_f16_issued / 1e9,
               "issued_f32_gflop_per_step": fam_f32_issued / 1e9, "algorithmic_gflop_per_step": fam_alg / 1e9,
               "frac_definition": "frac = the launches' matrix-pipe time at peak / their summed live duration: sum over launches of (FLOPs ISSUED / "
                                  "peak of the launch's operand type) - fp32 MFMA 157.3 TF for the stem (F(2,5) along x: 78/125 of the direct "
                                  "multiply-adds) and any fp32 Winograd launch (F(2x4,3x3): 1/3), f16 MFMA 2 500 TF for the f16x2 launches "
                                  "(csrc/conv3d_zw.hip: F(2,3) along z, 2/3 of the direct products, each cut into three fp16 products = 2 issued "
                                  "per algorithmic multiply-add).  achieved = frac x the f16 peak (f16-equivalent TFLOP/s).  "
                                  "frac_algorithmic = direct-convolution FLOPs (2*Cin*Cout*k^3 per voxel) over the same time / the fp32 "
                                  "peak: work delivered per fp32-peak-FLOP, > 1 is possible and is not a hardware fraction"}
    return fam, roofs


def bench_detect(args, rank, world, dist):
    import numpy as np
    import torch
    import m3d
    from m3d import shard
    from m3d.model import DetectorM3D, Probe
    from m3d.config import Cfg
    from m3d.synth import synth_volume

    backbone_only = args.workload == "backbone"
    subrecords = (not backbone_only) and world == 1 and not args.stress_rois and not args.no_subrecords
    cfg = Cfg.nuclei(in_size=(VOL, VOL, VOL))
    if args.stress_rois:
        cfg.rpn_nms_thresh = 1.0                       # nothing overlaps by more than 1: all RPN_POST_NMS_TOP_N = 1000 proposals survive
    P = cached_params(stride=8, num_anchors=35, mlp_dim=cfg.mlp_dim, seed=0, head=not backbone_only)
    det = DetectorM3D({k: v.cuda() for k, v in P.items()}, cfg)
    # 4 volumes per rank at EVERY N (configs[2] at N = 1): equal per-GPU work, so value(N) / (N * value(1)) is a weak-scaling efficiency
    nvol = args.vols_per_rank or (1 if backbone_only else 4)
    n_items = world * nvol
    nb = 1 if backbone_only else NB
    im_info = np.array([VOL, VOL, VOL, 1.0], np.float64)
    cap = cfg.detections_per_im
    last = {}
    rois_seen = []

    def make_batches(nv, nbatch):
        """Per-rank state for nv volumes per step and nbatch rotating batches: (batch function raw -> packed detections, raw volumes as
        ndarrays / pinned host tensors / device tensors (one per batch), fp32 work buffer)."""
        items = shard.partition(world * nv, rank, world)
        rnp = [np.stack([synth_volume(j * world * nv + i, (VOL, VOL, VOL)) for i in items]) for j in range(nbatch)]   # uint16, what io.imread gives
        rhost = [torch.from_numpy(a).pin_memory() for a in rnp]
        rdev = [h.cuda() for h in rhost]
        xb = torch.empty((nv, 1, VOL, VOL, VOL), dtype=torch.float32, device="cuda")

        def batch(raw, between=None):
            """The rank's batch of volumes -> packed detections [nv, cap+1, 7] on the device (m3d.shard block: rows = detections,
            trailer row = count).  norm1 per volume; ONE batched pass for the convolutions, RoIAlign and the box-head GEMMs; ONE
            launch each for the proposals, the per-class NMS + cap and the cross-tile NMS + packing of all volumes; one host read
            (the proposal counts that size the GEMM).  `between` (host-to-host loop): called when the backbone, RPN and proposal launches
            are queued and before the host waits for the proposal counts - where the next step's upload is issued."""
            if backbone_only:                                                           # configs[1]: the 3D-conv forward alone (xb was
                return det.conv_body(xb)                                                # normalised once, outside the timed steps)
            m3d.norm1_batched(raw, f32_arith=True, out=xb)                              # blob.py:179-184, per volume statistics
            st_ = det.detect_batch_begin(xb, im_info)                                   # core/test.py:106-114 per volume
            if between is not None:
                between()
            r = det.detect_batch_finish(st_, as_dicts=False)
            last["num_rois"] = r["num_rois"]
            rois_seen.append(float(sum(r["num_rois"])))
            if "cls_boxes" not in r:
                return torch.zeros((nv, cap + 1, 7), device="cuda")
            with det.span("cross_tile_nms_pack"):                                       # core/test.py:159 (one tile per volume) + pack
                return m3d.nms3d_batched(r["cls_boxes"][:, 1], r["cls_counts"][:, 1], cfg.nms, pack_cap=cap, want_keep=False)["packed"]
        return batch, rnp, rhost, rdev, xb

    batch, raw_np, raw_host, raw_dev, xbuf = make_batches(nvol, nb)
    if backbone_only:
        m3d.norm1_batched(raw_dev[0], f32_arith=True, out=xbuf)

    # `--backend gloo` (rehearsal of the N > 1 code path on a one-GPU box: ranks share the card, the exchange goes through host
    # memory) moves the packed block to the CPU for the collective; nccl (RCCL over xGMI) gathers device to device.
    via_host = dist is not None and args.backend == "gloo"

    def exchange(packed, items=None):
        return shard.all_gather_packed(packed.cpu() if via_host else packed, items or n_items, dist)   # THE exchange

    # HIP-event spans (Probe) ride on the first PROBE_STEPS steps of the timed region only: a probed step records ~40 timing events
    # between its kernels (+0.2 ms, 4 %), and past a few hundred live events the cost grows.  Warm-up steps carry a throw-away probe
    # (first launches, allocator growth and the event pool all belong to the caller's W warm-up steps: nothing runs before them).
    probed = {"probe": None, "left": 0}

    def arm(probe, steps):
        probed["probe"], probed["left"] = probe, steps

    def set_probe():
        det.probe = probed["probe"] if probed["left"] > 0 else None
        probed["left"] -= 1

    rk = {"i": 0}

    def step_resident():
        set_probe()
        b = rk["i"] % nb
        rk["i"] += 1
        packed = batch(raw_dev[b])
        if backbone_only:
            last["feat"] = packed
            return packed
        last["packed"] = exchange(packed)
        return last["packed"]

    # ---- host to host (`value` of the detect workloads): pinned raw volumes -> H2D on a copy stream (double-buffered) -> step
    # -> D2H of the gathered detections (double-buffered pinned outputs)
    if not backbone_only:
        copy_stream = torch.cuda.Stream()
        bufs = [torch.empty_like(raw_dev[0]) for _ in range(2)]
        ready = [torch.cuda.Event() for _ in range(2)]
        freed = [torch.cuda.Event() for _ in range(2)]
        host_out = [torch.empty((world, nvol, cap + 1, 7), dtype=torch.float32).pin_memory() for _ in range(2)]
        landed = [torch.cuda.Event() for _ in range(2)]
        state = {"i": 0}

        def upload(slot, which):
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(freed[slot])
                bufs[slot].copy_(raw_host[which % nb], non_blocking=True)
                ready[slot].record(copy_stream)

        for b_ in range(2):
            freed[b_].record()
        upload(0, 0)

        def step_host():
            hstamps.append(time.perf_counter())
            set_probe()
            i = state["i"]
            b = i & 1
            state["i"] += 1
            torch.cuda.current_stream().wait_event(ready[b])
            # the NEXT step's volumes (the next of the rotating batches) cross PCIe during this step.  On this stack the 16.8 MB pinned
            # hipMemcpyAsync holds the calling thread for ~0.5 ms: issued before the step's launches it kept the GPU waiting for them.
            # --upload-at end (rounds 4-5): after ALL of the step's launches - the copy then runs beside the box head (fc1 streams 0.8 GB)
            # and the next step's first kernels; --upload-at mid (round 6): once backbone / RPN / proposals are queued, before the host
            # waits for the proposal counts - the held thread is hidden behind 2.7 ms of queued convolutions and the copy runs beside them.
            # Measured equal (3.944 vs 3.940 ms per step, two runs each on one box): the 0.15 ms between this loop and `resident` is not a
            # matter of WHICH kernels the copy runs beside
            if args.upload_at == "mid":
                packed = batch(bufs[b], between=lambda: upload(b ^ 1, i + 1))
                freed[b].record()
            else:
                packed = batch(bufs[b])
                freed[b].record()
                upload(b ^ 1, i + 1)
            g = exchange(packed)
            last["packed"] = g
            if rank == 0:
                # outputs double-buffered like the inputs: this step's detections start their way to the host, the host waits for the
                # PREVIOUS step's (a full drain per step would leave the GPU idle while the next step is being launched: +0.25 ms);
                # the loop's closing synchronize lands the last ones inside the timed region
                host_out[b].copy_(g, non_blocking=True)
                landed[b].record()
                if i > 0:
                    landed[b ^ 1].synchronize()
            return g

    hstamps = []
    headline = step_resident if backbone_only else step_host
    arm(Probe(), args.warmup)                              # throw-away probe on the warm-up steps
    for _ in range(args.warmup):
        headline()
    torch.cuda.synchronize()
    # everything built so far (torch's module graph, the model, the batches: ~10^6 tracked objects) moves to the permanent generation:
    # a full collection that walks it takes 40-60 ms and would land in some 0.09 s timed region (the collector itself stays enabled)
    import gc
    gc.collect()
    gc.freeze()
    # The host-to-host loop runs BARE: a probed step records ~40 timing events between its kernels (5.0 instead of 4.4 ms per step, and the
    # steps behind it stay slow for a while); the rooflines' live spans come from the first PROBE_STEPS steps of the `resident` timed loop
    # below - the same K steps over the same batches.  (configs[1] has no resident loop: with --full its headline loop carries the probe.)
    main_probe = Probe()
    arm(main_probe, PROBE_STEPS if backbone_only and args.full else 0)
    del rois_seen[:]
    del hstamps[:]
    dt = timed_loop(headline, args.steps, 0, dist, torch.cuda.synchronize)
    step_ms_timed = [round((b_ - a_) * 1e3, 2) for a_, b_ in zip(hstamps[:-1], hstamps[1:])][:max(0, args.steps - 1)]
    dt = sync_max_time(dt, dist, "cpu" if via_host else "cuda")
    torch.cuda.synchronize()
    outputs = {"feat": last["feat"]} if backbone_only else {"detections": last["packed"]}     # the last timed step's, for --dump-outputs
    rois_per_step = float(np.mean(rois_seen)) if rois_seen else None
    res = {"metric": METRIC, "value": n_items * args.steps * VOL ** 3 / dt, "unit": "voxels/s", "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "f32", "data": "synthetic",
           "config": {"workload": ("dsn_body forward (7 conv3d + BN + ReLU + 3 maxpool; the volume normalised beforehand), 1x1x128x128x128 per rank [configs[1]]"
                                   if backbone_only else
                                   "detection-mode infer_simple, host to host: pinned raw u16 volumes -> H2D -> norm1 -> dsn_body -> RPN -> proposals "
                                   "-> RoIAlign3D -> 2-MLP head -> decode -> NMS -> cross-tile NMS -> one all_gather of detections -> D2H; batch of "
                                   "%d x (1x128^3) per rank, %d distinct batches rotating [%s]%s"
                                   % (nvol, nb, "configs[2]" if (world == 1 and nvol == 4) else "%d volumes over %d GPUs%s" %
                                      (n_items, world, " = configs[4]" if n_items == 64 and world == 8 else ""),
                                      " STRESS: RPN NMS off, %d RoIs per volume (RPN_POST_NMS_TOP_N)" % cfg.post_nms_topN if args.stress_rois else "")),
                      "volumes_per_step": n_items, "volumes_per_rank": nvol, "distinct_batches": nb,
                      "backend": (args.backend if world > 1 else None), "net": "nuclei stride-8 dsn_body, 35 anchors, MLP 1024",
                      "inputs": ("one normalised fp32 volume resident in HBM" if backbone_only else
                                 "raw uint16 volumes in pinned host memory at the start of the timed region; detections on the host at its end"),
                      "rois_per_volume": (rois_per_step / nvol if rois_per_step else None),
                      "dets_per_volume": (float(last["packed"][..., cap, 0].float().mean().item()) if "packed" in last else None)}}
    if not args.full:                            # a plain run: the headline alone
        return (res, outputs) if rank == 0 else (None, None)
    kern_ms = main_probe.mean_ms()
    kern_med = main_probe.median_ms()
    main_probe.spans.clear()                     # hand the timing events back to torch's pool: creating fresh ones (hipEventCreate with timing)
    det.probe = None                             # costs ~0.4 ms each - 120 of them made the next probed loop 2 ms per step slower
    arm(None, 0)
    rois_probed = float(np.mean(rois_seen[:PROBE_STEPS])) if rois_seen else None
    rmed = None

    # ---- the same steps with the raw volumes resident in HBM (the `value` of rounds 1-3)
    resident = None
    warm = None
    rkern = None
    if not backbone_only:
        for _ in range(2):
            step_resident()
        rprobe = Probe()
        arm(rprobe, PROBE_STEPS)
        n_seen = len(rois_seen)
        dtr = timed_loop(step_resident, args.steps, 0, dist, torch.cuda.synchronize)
        if len(rois_seen) > n_seen:
            rois_probed = float(np.mean(rois_seen[n_seen:n_seen + PROBE_STEPS]))       # the RoIs of the probed steps (fc1 / RoIAlign rooflines)
        dtr = sync_max_time(dtr, dist, "cpu" if via_host else "cuda")
        torch.cuda.synchronize()
        det.probe = None
        arm(None, 0)
        # two more passes of the same K steps: on these boxes a 40-60 ms stall lands somewhere in the ~0.3 s after the host-to-host loop
        # (seen in the first or the second pass, never in the >= 2 s sustained loop; its origin is outside this process' kernels).  The
        # headline region is what it is; this secondary figure lists all passes and uses the best
        res_runs = [dtr / args.steps * 1e3]
        for _ in range(2):
            d_ = timed_loop(step_resident, args.steps, 0, dist, torch.cuda.synchronize)
            d_ = sync_max_time(d_, dist, "cpu" if via_host else "cuda")
            res_runs.append(d_ / args.steps * 1e3)
            dtr = min(dtr, d_)
        # the host-to-host loop once more, now that the chip has been under load for a quarter of a second: what `value` would be without the
        # clock ramp of its first steps (config.step_ms_timed); W warm-up steps of its own, K steps, three passes
        for _ in range(args.warmup):
            step_host()
        warm_runs = []
        for _ in range(3):
            d_ = timed_loop(step_host, args.steps, 0, dist, torch.cuda.synchronize)
            d_ = sync_max_time(d_, dist, "cpu" if via_host else "cuda")
            warm_runs.append(d_)
        warm = {"value": n_items * args.steps * VOL ** 3 / min(warm_runs), "unit": "voxels/s", "ms_per_step": min(warm_runs) / args.steps * 1e3,
                "ms_per_step_runs": [round(d_ / args.steps * 1e3, 4) for d_ in warm_runs],
                "what": "the `value` loop (host to host, W warm-up steps, K timed steps) repeated after the resident passes, i.e. on a chip that "
                        "holds its clock; `value` itself is the first loop after the model build, as the bench contract times it"}
        rkern = rprobe.mean_ms()
        rmed = rprobe.median_ms()
        rfam, _ = conv_family_roofline(det, det.conv_work(nvol, (VOL, VOL, VOL)), rkern, nvol, "the rank's batch of %d volumes" % nvol)
        rprobe.spans.clear()
        resident = {"value": n_items * args.steps * VOL ** 3 / dtr, "unit": "voxels/s", "ms_per_step": dtr / args.steps * 1e3,
                    "ms_per_step_runs": [round(r_, 4) for r_ in res_runs],
                    "roofline": None if rfam is None else {k: rfam[k] for k in ("bound", "achieved", "peak", "unit", "frac", "frac_algorithmic", "kernel_ms")},
                    "roofline_note": "the conv family's spans in THIS loop: no upload runs beside the kernels (in the host-to-host loop the next "
                                     "batch's 16.8 MB H2D copy shares HBM and power with them)",
                    "what": "the same %d steps over the same rotating batches with the raw uint16 volumes already in HBM and the "
                            "detections left on the device (the definition of `value` in rounds 1-3)" % args.steps}

    # ---- (1b) the same K steps software-pipelined over two streams / (1c) interleaved on one stream: opt-in, N = 1
    def run_finish(prev):
        r = det.detect_batch_finish(prev, as_dicts=False)
        packed = (m3d.nms3d_batched(r["cls_boxes"][:, 1], r["cls_counts"][:, 1], cfg.nms, pack_cap=cap, want_keep=False)["packed"]
                  if "cls_boxes" in r else torch.zeros((nvol, cap + 1, 7), device="cuda"))
        return exchange(packed)

    def measure_pipelined():
        sA, sB = torch.cuda.Stream(), torch.cuda.Stream()
        xb2 = [xbuf, torch.empty_like(xbuf)]

        def run_pipelined(n):
            prev, st = None, None
            for i in range(n + 1):
                if i < n:
                    with torch.cuda.stream(sA):
                        m3d.norm1_batched(raw_dev[i % nb], f32_arith=True, out=xb2[i & 1])
                        st = det.detect_batch_begin(xb2[i & 1], im_info)
                if prev is not None:
                    with torch.cuda.stream(sB):
                        last["packed_pipelined"] = run_finish(prev)
                prev = st if i < n else None
        torch.cuda.synchronize()
        run_pipelined(2)
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):                               # three repeats: the overlap depends on how the two streams' kernels meet
            t0 = time.perf_counter()
            run_pipelined(args.steps)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / args.steps * 1e3)
        ms = sorted(runs)[1]
        return {"value": n_items * VOL ** 3 / (ms * 1e-3), "unit": "voxels/s", "ms_per_step": ms, "ms_per_step_runs": [round(r, 4) for r in runs],
                "what": "the resident steps with begin(k+1) (norm1, backbone, RPN, proposals) launched on a second stream before "
                        "finish(k) (RoIAlign, box head, box results, cross-tile NMS, exchange); median of three repeats"}

    def measure_interleaved():
        xb2 = [xbuf, torch.empty_like(xbuf)]

        def run(n):
            m3d.norm1_batched(raw_dev[0], f32_arith=True, out=xb2[0])
            st = det.detect_batch_begin(xb2[0], im_info)
            for k in range(n):
                nxt = None
                if k + 1 < n:
                    m3d.norm1_batched(raw_dev[(k + 1) % nb], f32_arith=True, out=xb2[(k + 1) & 1])
                    nxt = det.detect_batch_begin(xb2[(k + 1) & 1], im_info)
                last["packed_interleaved"] = run_finish(st)
                st = nxt
        torch.cuda.synchronize()
        run(2)
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            run(args.steps)
            torch.cuda.synchronize()
            runs.append((time.perf_counter() - t0) / args.steps * 1e3)
        ms = sorted(runs)[1]
        return {"value": n_items * VOL ** 3 / (ms * 1e-3), "unit": "voxels/s", "ms_per_step": ms, "ms_per_step_runs": [round(r, 4) for r in runs],
                "what": "the resident steps on one stream with begin(k+1) (norm1, backbone, RPN, proposals) enqueued before the host "
                        "reads the proposal counts of batch k; median of three repeats"}

    inter = piped = None
    if not backbone_only and world == 1:
        for flag, fn, key in ((args.interleaved, measure_interleaved, "inter"), (args.pipelined, measure_pipelined, "piped")):
            if not flag:
                continue
            try:
                r_ = fn()
            except Exception as e:                       # an opt-in extra must not lose the main line
                r_ = {"error": "%s: %s" % (type(e).__name__, e)}
                torch.cuda.synchronize()
            if key == "inter":
                inter = r_
            else:
                piped = r_

    # ---- sustained: the resident loop again for at least two seconds (the timed regions above last ~0.1 s)
    sustained = None
    if not backbone_only:
        per = resident["ms_per_step"] * 1e-3
        n_sus = max(args.steps, int(2.0 / max(per, 1e-6)) + 1)            # the same count on every rank (per is the max over ranks)
        dts = timed_loop(step_resident, n_sus, 0, dist, torch.cuda.synchronize)
        dts = sync_max_time(dts, dist, "cpu" if via_host else "cuda")
        sustained = {"value": n_items * n_sus * VOL ** 3 / dts, "unit": "voxels/s", "ms_per_step": dts / n_sus * 1e3, "steps": n_sus,
                     "seconds": dts}

    # ---- N > 1: what the scaling ratio is made of.  (a) the same per-rank batches WITHOUT the exchange; (b) rank 0's batch alone
    # on its GPU while the other ranks wait (a single-GPU run of the same batch inside this job); (c) the all_gather alone;
    # (d) BASELINE configs[4]'s shape (8 volumes per rank) when this run uses another batch
    no_xchg = same_batch = xchg = cfg4 = None
    if dist is not None and not backbone_only:
        cnt = {"i": 0}

        def step_no_x():
            cnt["i"] += 1
            return batch(raw_dev[cnt["i"] % nb])
        dt3 = timed_loop(step_no_x, args.steps, 1, dist, torch.cuda.synchronize)
        dt3 = sync_max_time(dt3, dist, "cpu" if via_host else "cuda")
        no_xchg = {"value": n_items * args.steps * VOL ** 3 / dt3, "unit": "voxels/s", "ms_per_step": dt3 / args.steps * 1e3,
                   "what": "all ranks' resident batches of %d volumes, no all_gather (max over ranks)" % nvol}
        dist.barrier()
        if rank == 0:
            dt4 = timed_loop(step_no_x, args.steps, 1, None, torch.cuda.synchronize)
            same_batch = {"value": nvol * args.steps * VOL ** 3 / dt4, "unit": "voxels/s", "ms_per_step": dt4 / args.steps * 1e3,
                          "what": "rank 0's resident batches of %d volumes alone (the other ranks wait at a barrier): the single-GPU rate "
                                  "of the same per-rank work, measured inside this job" % nvol}
        dist.barrier()
        packed0 = batch(raw_dev[0])
        torch.cuda.synchronize()
        nx = 50
        dt5 = timed_loop(lambda: exchange(packed0), nx, 5, dist, torch.cuda.synchronize)
        dt5 = sync_max_time(dt5, dist, "cpu" if via_host else "cuda")
        xchg = {"us": dt5 / nx * 1e6, "microseconds_per_all_gather": dt5 / nx * 1e6, "ranks": dist.get_world_size(), "backend": dist.get_backend(),
                "bytes_per_rank": int(nvol * (cap + 1) * 7 * 4),
                "what": "one all_gather_into_tensor of the packed [%d,%d,7] block per rank, issued back to back" % (nvol, cap + 1)}
        if nvol != 8:
            b8, _, _, rdev8, _ = make_batches(8, 1)
            dt6 = timed_loop(lambda: exchange(b8(rdev8[0]), world * 8), args.steps, 2, dist, torch.cuda.synchronize)
            dt6 = sync_max_time(dt6, dist, "cpu" if via_host else "cuda")
            cfg4 = {"value": world * 8 * args.steps * VOL ** 3 / dt6, "unit": "voxels/s", "ms_per_step": dt6 / args.steps * 1e3,
                    "volumes_per_rank": 8, "volumes_per_step": world * 8,
                    "what": "BASELINE configs[4]'s partition (8 volumes per rank; 64 over 8 GPUs), resident inputs, with the exchange"}

    # ---- sub-records measured with THIS detector (N = 1, default workload): the stress step and configs[1]
    stress = bb1 = None
    if subrecords:
        # (a) RPN NMS off: RPN_POST_NMS_TOP_N = 1000 proposals per volume reach the box head (the synthetic weights' own RPN NMS keeps ~320)
        keep_thr = cfg.rpn_nms_thresh
        cfg.rpn_nms_thresh = 1.0
        try:
            n0 = len(rois_seen)
            for _ in range(3):
                step_resident()
            sp = Probe()
            arm(sp, PROBE_STEPS)
            ns = max(6, args.steps // 2)
            del rois_seen[:]
            dt_s = timed_loop(step_resident, ns, 0, None, torch.cuda.synchronize)
            torch.cuda.synchronize()
            km = sp.mean_ms()
            sp.spans.clear()
            det.probe = None
            arm(None, 0)
            Rs = float(np.mean(rois_seen)) if rois_seen else 0.0
            ra_bytes = Rs * 256 * 343 * 4.0
            stress = {"value": nvol * ns * VOL ** 3 / dt_s, "unit": "voxels/s", "ms_per_step": dt_s / ns * 1e3, "steps": ns, "warmup": 3,
                      "config": {"workload": "the default detect step (resident inputs, rotating batches) with the RPN NMS threshold at 1.0: "
                                             "every volume hands RPN_POST_NMS_TOP_N = %d RoIs to the box head" % cfg.post_nms_topN,
                                 "rois_per_volume": Rs / nvol, "kernel_ms_per_launch": {k: round(v, 4) for k, v in sorted(km.items(), key=lambda kv: -kv[1])}},
                      "roofline": ({"bound": "hbm", "kernel": "roi_align3d_fwd_v3_kernel (RoIAlign3D forward, the step's HBM-write-bound launch)",
                                    "achieved": ra_bytes / (km["roi_align3d"] * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                    "frac": ra_bytes / (km["roi_align3d"] * 1e-3) / 1e9 / HBM_PEAK_GBS, "kernel_ms": km["roi_align3d"],
                                    "algorithmic_bytes_per_launch": ra_bytes,
                                    # PMC pass of the same stress step (tools/pmc_probe.py, the launch with the largest grid)
                                    "traffic": pmc_traffic("roi_align3d_fwd_v3_kernel", which="largest").get("traffic")}
                                   if "roi_align3d" in km else None)}
            del n0
        finally:
            cfg.rpn_nms_thresh = keep_thr
        # (b) configs[1]: dsn_body forward alone, ONE 1x128^3 volume per launch
        x1 = xbuf[:1].contiguous()
        m3d.norm1_batched(raw_dev[0][:1].contiguous(), f32_arith=True, out=x1)
        for _ in range(20):
            det.conv_body(x1)
        bp = Probe()
        kb = {"left": PROBE_STEPS}

        def step_bb():
            det.probe = bp if kb["left"] > 0 else None
            kb["left"] -= 1
            return det.conv_body(x1)
        nsb = 100
        dt_b = timed_loop(step_bb, nsb, 0, None, torch.cuda.synchronize)
        torch.cuda.synchronize()
        det.probe = None
        kmb = bp.mean_ms()
        bp.spans.clear()
        fam_b, roofs_b = conv_family_roofline(det, det.conv_work(1, (VOL, VOL, VOL)), kmb, 1, "one 1x128^3 volume")
        if fam_b is not None and "conv2b" in roofs_b:
            if "f16x2" in roofs_b["conv2b"]["kernel"]:          # persistent launches: one grid for every layer and batch size - no per-batch-size record
                fam_b["traffic"] = None
            else:
                fam_b.update(pmc_traffic("conv3d_wino24_kernel<4, 16, 2, 1, true", grid_div=nvol))
                fam_b["traffic_what"] = "HBM bytes per launch of the largest member (conv2b + pool) at this batch size, PMC"
        bb1 = {"value": nsb * VOL ** 3 / dt_b, "unit": "voxels/s", "ms_per_step": dt_b / nsb * 1e3, "steps": nsb, "warmup": 20,
               "config": {"workload": "dsn_body forward (7 conv3d + BN + ReLU + 3 maxpool; the volume normalised beforehand), 1x1x128x128x128 [configs[1]]",
                          "backbone_gflop_per_volume": backbone_flops(VOL) / 1e9,
                          "backbone_algorithmic_tflops": backbone_flops(VOL) / (dt_b / nsb) / 1e12,
                          "kernel_ms_per_launch": {k: round(v, 4) for k, v in sorted(kmb.items(), key=lambda kv: -kv[1])}},
               "roofline": fam_b, "rooflines": roofs_b}

    if rank != 0:
        return None, None
    # ---- rooflines from the live HIP-event spans of the timed region.  `roofline` = the 3D-convolution family, the quantity the metric
    # names: MFMA FLOPs issued by all its launches over their summed duration; `rooflines` = one entry per conv layer + fc1
    wino = det.wino_mode
    if rkern:                                    # the detect workloads: every span comes from the resident timed loop (the headline loop runs bare)
        kern_ms, kern_med = rkern, (rmed or rkern)
    kern = {k: round(v, 4) for k, v in sorted(kern_ms.items(), key=lambda kv: -kv[1])}
    work = det.conv_work(nvol, (VOL, VOL, VOL))
    # the spans of the RESIDENT loop feed the rooflines: in the host-to-host loop the launching thread also issues the pinned uploads
    # (~0.5 ms of host time per step), launches arrive late and an event span then holds queue idle time as well as the kernel
    # (conv family 2.95 ms by those spans against 2.69 ms by rocprofv3's kernel trace and 2.7 ms by the resident spans)
    span_ms = rkern if rkern else kern_ms
    conv_family, roofs = conv_family_roofline(det, work, span_ms, nvol, "the rank's batch of %d volumes" % nvol)
    if conv_family is not None:
        conv_family["region"] = ("HIP-event spans of the first %d steps of the `resident` timed loop (same kernels, same K steps, same batches); the "
                                 "host-to-host loop that gives `value` carries no probe" % PROBE_STEPS) \
            if rkern else "HIP-event spans of the first %d timed steps" % PROBE_STEPS
    if "conv2b" in roofs:
        w2 = "conv3d_zw_kernel<32, true" if "f16x2" in work["conv2b"]["kernel"] else \
            "conv3d_wino24_kernel<4, 16, 2, 1, true" if "F(2x4" in work["conv2b"]["kernel"] else "conv3d_wino2e_kernel<4, 32, 2, 2, true>"
        roofs["conv2b"].update(pmc_traffic({2: w2, 1: "conv3d_wino_kernel<4, 32, 1, 2, 2, 4, 1, true>",
                                            0: "conv3d_mfma_kernel<3, 2, 32, 4, 2, 2, 2, true, 1>"}[wino]))
    if conv_family is not None:
        conv_family["traffic"] = (roofs.get("conv2b", {}) or {}).get("traffic")
        conv_family["traffic_what"] = "HBM bytes per launch of the largest member (conv2b), PMC: " + str((roofs.get("conv2b", {}) or {}).get("traffic_source"))
    if "fc1" in span_ms and rois_probed:
        ms = span_ms["fc1"]
        M = int(round(rois_probed))
        Kf, Nf = 256 * 343, cfg.mlp_dim
        fl = 2.0 * M * Nf * Kf
        import m3d.ops as _ops
        if isinstance(getattr(det, "fc_split", {}).get("fc1"), _ops.SplitLinearF16):
            # f16x2 split (round 6): three f16 MFMAs per fp32 multiply-add (two scaled fp16 planes per operand) -> priced against the f16 / bf16 peak
            r = {"bound": "mfma", "launch": "one launch over the RoIs of the rank's %d volumes (M = %d rows, mean of the probed steps)" % (nvol, M),
                 "kernel": "fc_x3b_gemm_kernel<1> (Box_Head.fc1: [M,87808] x [1024,87808]^T on v_mfma_f32_32x32x16_f16: both operands scaled by a power "
                           "of two and cut into two fp16 numbers (22 bits), 3 products per fp32 product, 256 x 256 tiles, split-K; + absmax of the "
                           "feature map (the x scale) + fc_reduce_kernel in the same span)",
                 "achieved": 3.0 * fl / (ms * 1e-3) / 1e12, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                 "frac": 3.0 * fl / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, "kernel_ms": ms,
                 "issued_gflop_per_launch": 3.0 * fl / 1e9, "algorithmic_gflop_per_launch": fl / 1e9,
                 "algorithmic_equivalent_tflops": fl / (ms * 1e-3) / 1e12,
                 "fp32_mfma_peak_multiple": fl / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                 "ceiling_tflops": BF16_MFMA_PEAK_TFLOPS / 3.0,
                 "frac_of_ceiling": fl / (ms * 1e-3) / 1e12 / (BF16_MFMA_PEAK_TFLOPS / 3.0),
                 "algorithmic_bytes_per_launch": M * Kf * 4.0 + Nf * Kf * 4.0 + M * Nf * 4.0,
                 "note": "achieved/frac count the f16 MFMA FLOPs ISSUED (3 x 2MNK) against the dense f16 (= bf16) peak; "
                         "algorithmic_equivalent_tflops = 2MNK / time.  Error vs fp64 on this shape equals the fp32-input kernel's "
                         "(tests/test_gpu_ops.py: test_linear_f16x2_split_gemm_is_as_accurate_as_the_fp32_kernel); M3D_FC_SPLIT=bf16x3 selects "
                         "round 2-5's exact 3-way bf16 cut (6 products)"}
            r.update(pmc_traffic("fc_x3b_gemm_kernel<1>"))
        elif "fc1" in getattr(det, "fc_split", {}):
            # bf16x3 split: six bf16 MFMAs per fp32 multiply-add (exact 3-way cut of both operands) -> priced against the bf16 peak
            r = {"bound": "mfma", "launch": "one launch over the RoIs of the rank's %d volumes (M = %d rows, mean of the probed steps)" % (nvol, M),
                 "kernel": "fc_x3_gemm_kernel (Box_Head.fc1: [M,87808] x [1024,87808]^T at fp32 accuracy on v_mfma_f32_32x32x16_bf16: "
                           "exact 3-way bf16 cut of x and W, 6 products per fp32 product, split-K; + fc_reduce_kernel; <= 64 rows past a multiple of the "
                           "256-row tile go through fc_gemm_kernel's ragged-tile path in the same span)",
                 "achieved": 6.0 * fl / (ms * 1e-3) / 1e12, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                 "frac": 6.0 * fl / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, "kernel_ms": ms,
                 "issued_gflop_per_launch": 6.0 * fl / 1e9, "algorithmic_gflop_per_launch": fl / 1e9,
                 "algorithmic_equivalent_tflops": fl / (ms * 1e-3) / 1e12,
                 "fp32_mfma_peak_multiple": fl / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS,
                 "ceiling_tflops": BF16_MFMA_PEAK_TFLOPS / 6.0,
                 "frac_of_ceiling": fl / (ms * 1e-3) / 1e12 / (BF16_MFMA_PEAK_TFLOPS / 6.0),
                 "algorithmic_bytes_per_launch": M * Kf * 4.0 + Nf * Kf * 6.0 + M * Nf * 4.0,
                 "note": "achieved/frac count the bf16 MFMA FLOPs ISSUED (6 x 2MNK) against the dense bf16 peak; "
                         "algorithmic_equivalent_tflops = 2MNK / time, fp32_mfma_peak_multiple = that over the 157.3 TF fp32-input MFMA "
                         "peak the round-1 kernel was bound by.  Error vs fp64 equals the fp32 kernel's (tests/test_gpu_ops.py)"}
            r.update(pmc_traffic("fc_x3_gemm_kernel"))
        else:
            r = {"bound": "mfma", "launch": "one launch over the RoIs of the rank's %d volumes (M = %d rows)" % (nvol, M),
                 "kernel": "fc_gemm_kernel (Box_Head.fc1: [M,87808] x [1024,87808]^T, split-K fp32 MFMA GEMM; + fc_reduce_kernel)",
                 "achieved": fl / (ms * 1e-3) / 1e12, "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                 "frac": fl / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, "kernel_ms": ms, "algorithmic_gflop_per_launch": fl / 1e9,
                 "algorithmic_bytes_per_launch": (M + Nf) * Kf * 4.0 + M * Nf * 4.0,
                 "note": "every multiply-add of the GEMM is issued (no Winograd): achieved = 2*M*N*K / time of the GEMM + its split-K reduction"}
            r.update(pmc_traffic("fc_gemm_kernel"))
        roofs["fc1"] = r
    if "roi_align3d" in span_ms and rois_probed:
        ms = span_ms["roi_align3d"]
        byt = rois_probed * 256 * 343 * 4.0
        r = {"bound": "hbm", "kernel": "roi_class_kernel + roi_align3d_fwd_v3_kernel (+ complement pass)", "achieved": byt / (ms * 1e-3) / 1e9,
             "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": byt / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "kernel_ms": ms,
             "algorithmic_bytes_per_launch": byt}
        r.update(pmc_traffic("roi_align3d_fwd_v3_kernel"))
        roofs["roi_align3d"] = r
    body_ms = sum(v for k, v in kern_ms.items() if k.startswith("conv")) / nvol      # spans cover the whole batch
    res["config"].update({
                      "backbone_gflop_per_volume": backbone_flops(VOL) / 1e9, "backbone_ms_per_volume": body_ms,
                      "backbone_algorithmic_tflops": backbone_flops(VOL) / (body_ms * 1e-3) / 1e12 if body_ms else None,
                      "kernel_ms_per_launch": kern,
                      "warmup_note": "exactly the caller's W warm-up steps run before the timed region (they carry a throw-away event probe); "
                                     "no hidden initialisation steps",
                      "kernel_ms_source": ("HIP-event spans on the launch stream, first %d of the %d steps of the `resident` timed loop (a probed step carries "
                                           "~40 event records and runs 5.0 instead of 4.4 ms; the host-to-host loop runs bare)" if rkern else
                                           "HIP-event spans on the launch stream, first %d of the %d timed steps") % (min(PROBE_STEPS, args.steps), args.steps),
                      "step_ms_timed": step_ms_timed,
                      "step_ms_timed_note": "host-side period of the timed steps of the `value` loop (the host waits inside every step, so it follows the "
                                            "GPU).  The first ~8 are slow: the chip is still coming up to its clock after the W warm-up steps "
                                            "(process start and model build leave it idle); with half a second of GPU load in front of the warm-up "
                                            "every timed step ran 4.3-4.45 ms and the loop 4.37 (measured, not done here: no hidden warm-up) - "
                                            "`warm_host_to_host` is the same loop on a chip that holds its clock, `sustained` the steady state of the resident steps",
                      "kernel_ms_per_launch_median": {k: round(v, 4) for k, v in sorted(kern_med.items(), key=lambda kv: -kv[1])}})
    res.update(roofline=conv_family, rooflines=roofs)
    if getattr(det, "conv_f16", False) or (not backbone_only and getattr(det, "fc_split", None)):
        res["dtype_note"] = ("every operand, accumulator and result is fp32; " + ("the 3^3 conv layers with 16 | cin (conv2a .. conv4b, the RPN conv) and " if getattr(det, "conv_f16", False) else "") +
                             "fc1 / fc2 multiply on the f16 matrix cores after both fp32 operands are scaled "
                             "by a power of two and cut into two fp16 numbers (22 significand bits; 3 MFMAs per product, fp32 accumulation; error vs "
                             "fp64 on the shipped shape = the fp32-input kernel's, tests/test_gpu_ops.py); M3D_FC_SPLIT=bf16x3 selects the exact "
                             "3-way bf16 cut (6 MFMAs, rounds 2-5), M3D_FC_SPLIT=0 the fp32-input MFMA kernel")
    for k, v in (("resident", resident), ("warm_host_to_host", warm), ("sustained", sustained), ("pipelined", piped), ("interleaved", inter)):
        if v is not None:
            res[k] = v
    res["value_definition"] = ("voxels of all volumes of the step / wall time of the timed steps; " +
                               ("one normalised volume resident in HBM (configs[1] names the conv forward alone)" if backbone_only else
                                "SURVEY 8d host to host: raw uint16 volumes start in pinned host memory, the gathered detections end on the host "
                                "(`resident`: the same steps with the inputs already in HBM, 1-3 % faster)"))
    for k, v in (("without_exchange", no_xchg), ("single_gpu_same_batch", same_batch), ("exchange", xchg), ("configs4_shape", cfg4)):
        if v is not None:
            res[k] = v
    if not args.no_cpu_baseline and world == 1 and not args.stress_rois:      # contract: CPU baseline on rank 0 at N = 1 only
        # CPU baseline leg: the ONLY place bench.py touches oracle/ (the checker's restatement of the same per-volume pipeline)
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle as O
        ncpu = host_cores()
        torch.set_num_threads(ncpu)
        ocfg = O.Cfg()

        def cpu_volume(raw, body_only):
            x = torch.from_numpy(O.norm1(raw, np.float32).astype(np.float32)).view(1, 1, VOL, VOL, VOL)
            with torch.no_grad():
                if body_only:
                    return O.dsn_body_forward(P, x, 8)
                r = O.detect_tile(P, ocfg, x)
            d = r["cls_boxes"][1]
            return d[O.nms_3d(np.ascontiguousarray(d, dtype=np.float32), ocfg.nms)] if len(d) else d
        flat = [v for b_ in raw_np for v in b_]
        cpu_volume(flat[0], backbone_only)           # warm-up (thread pool, page-in)
        nrep, tcpu = 0, 0.0
        while tcpu < 12.0 and nrep < 8:
            c0 = time.perf_counter()
            cpu_volume(flat[nrep % len(flat)], backbone_only)
            tcpu += time.perf_counter() - c0
            nrep += 1
        res["cpu_baseline"] = {"value": nrep * VOL ** 3 / tcpu, "unit": "voxels/s", "cores": ncpu, "kind": "port",
                               "sample": "%d of the same 1x128^3 volumes through the oracle's restatement of the same pipeline (NumPy norm1, "
                                         "torch-CPU fp32 convs/linears with %d threads, oracle C proposals/RoIAlign/NMS on 1 thread), %.1f s"
                                         % (nrep, ncpu, tcpu)}
        res["speedup_vs_cpu_baseline"] = res["value"] / res["cpu_baseline"]["value"]
        if bb1 is not None:                          # configs[1]'s own CPU leg: the conv forward alone
            nrep, tcpu = 0, 0.0
            while tcpu < 3.0 and nrep < 6:
                c0 = time.perf_counter()
                cpu_volume(flat[nrep % len(flat)], True)
                tcpu += time.perf_counter() - c0
                nrep += 1
            bb1["cpu_baseline"] = {"value": nrep * VOL ** 3 / tcpu, "unit": "voxels/s", "cores": ncpu, "kind": "port",
                                   "sample": "%d x dsn_body forward of a 1x128^3 volume, torch-CPU fp32 with %d threads (oracle.dsn_body_forward), %.1f s"
                                             % (nrep, ncpu, tcpu)}
    if bb1 is not None:
        res["configs1_backbone"] = bb1
    if stress is not None:
        res["stress_rois"] = stress
    return res, outputs


def condensed(r):
    """A sub-record of the default line: what the judge reads (value, ms_per_step, roofline, cpu_baseline, the workload)."""
    if r is None:
        return None
    keep = ("value", "unit", "ms_per_step", "ms_per_step_median", "steps", "warmup", "roofline", "cpu_baseline", "speedup_vs_cpu_baseline", "otsu", "volumes")
    out = {k: r[k] for k in keep if k in r}
    out["config"] = {k: v for k, v in r.get("config", {}).items() if k in ("workload", "peaks_per_tile", "phase_ms", "prm_forward_ms", "prm_backward_ms",
                                                                             "rois_per_volume", "instances_painted", "launches_per_tile", "peaks_back_propagated")}
    return out


# ------------------------------------------------------------------------------------------------ the ONE stdout line
LINE_MAX = 8000        # the driver keeps ~9 KB of stdout tail: a longer final line cannot be parsed (round 4: 25.9 KB -> `parsed: null`)
ROOF_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "frac_algorithmic", "kernel_ms", "traffic")
CPU_KEYS = ("value", "unit", "cores", "kind", "sample")


def _num(x, sig=6):
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float("%.*g" % (sig, x))


def _txt(s, n):
    return s if len(s) <= n else s[:n - 3] + "..."


def _pick(d, keys, text=100):
    if not isinstance(d, dict):
        return None
    return {k: (_txt(d[k], text) if isinstance(d[k], str) else _num(d[k])) for k in keys if k in d}


def compact_line(res, full_path=None):
    """The final stdout line: contract keys, `roofline`, `cpu_baseline`, and for every sub-record only value / ms_per_step /
    roofline.frac+traffic / cpu_baseline.value / config.workload.  Everything else lives in the full record (stderr + `full_path`).
    Always json-parseable and shorter than LINE_MAX (tests/test_bench_line.py)."""
    top = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "dry")
    out = {k: _num(res[k], 17) for k in top if k in res}
    cfg = res.get("config", {}) or {}
    out["config"] = {k: (_txt(v, 330) if isinstance(v, str) else _num(v)) for k, v in cfg.items()
                     if k in ("workload", "volumes_per_step", "volumes_per_rank", "rois_per_volume", "dets_per_volume", "backend", "peaks_per_tile")
                     and v is not None}
    if res.get("roofline") is not None:
        out["roofline"] = _pick(res["roofline"], ROOF_KEYS, 150)
    elif "roofline" in res:
        out["roofline"] = None
    if res.get("cpu_baseline") is not None:
        out["cpu_baseline"] = _pick(res["cpu_baseline"], CPU_KEYS, 220)
        if "speedup_vs_cpu_baseline" in res:
            out["speedup_vs_cpu_baseline"] = _num(res["speedup_vs_cpu_baseline"], 4)
    for k in ("resident", "warm_host_to_host", "sustained", "without_exchange", "single_gpu_same_batch", "configs4_shape", "pipelined", "interleaved"):
        if isinstance(res.get(k), dict):
            out[k] = _pick(res[k], ("value", "ms_per_step", "volumes_per_step", "volumes_per_rank"))
    if isinstance(res.get("exchange"), dict):
        out["exchange"] = _pick(res["exchange"], ("us", "ranks", "backend", "bytes_per_rank", "collective"), 60)
    for k in ("configs1_backbone", "stress_rois", "configs3_prm_soma", "prm_nuclei_tile", "volume_pipeline"):
        r = res.get(k)
        if not isinstance(r, dict):
            continue
        if "error" in r:
            out[k] = {"error": _txt(str(r["error"]), 200)}
            continue
        sub = {"value": _num(r.get("value")), "ms_per_step": _num(r.get("ms_per_step"))}
        if isinstance(r.get("roofline"), dict):
            sub["roofline"] = _pick(r["roofline"], ("bound", "kernel", "frac", "frac_algorithmic", "kernel_ms", "traffic"), 90)
        else:
            sub["roofline"] = None
        if isinstance(r.get("cpu_baseline"), dict):
            sub["cpu_baseline"] = _pick(r["cpu_baseline"], ("value", "cores", "kind"))
        c = r.get("config", {}) or {}
        sub["config"] = {kk: (_txt(v, 150) if isinstance(v, str) else _num(v)) for kk, v in c.items()
                         if kk in ("workload", "peaks_per_tile", "peaks_back_propagated", "rois_per_volume", "prm_backward_ms", "prm_forward_ms", "launches_per_tile")
                         and v is not None}
        if isinstance(r.get("volumes"), dict):
            sub["volumes"] = {n: _pick(v, ("value", "seconds_per_volume", "peaks", "peaks_back_propagated")) for n, v in r["volumes"].items() if isinstance(v, dict)}
        out[k] = sub
    if res.get("accounting_errors"):
        out["accounting_errors"] = [_txt(str(e), 120) for e in res["accounting_errors"][:4]]
    if full_path:
        out["full_record"] = full_path
    line = json.dumps(out)
    if len(line) >= LINE_MAX:                        # cannot happen with the caps above; never emit an unparseable line
        for k in ("volume_pipeline", "prm_nuclei_tile", "configs3_prm_soma", "stress_rois", "configs1_backbone", "sustained", "warm_host_to_host"):
            if k in out and len(line) >= LINE_MAX:
                out[k] = {"value": (out[k] or {}).get("value"), "ms_per_step": (out[k] or {}).get("ms_per_step")}
                line = json.dumps(out)
    assert len(line) < LINE_MAX, len(line)
    return line


def hardware_fracs_above_one(rec, path=""):
    """Every `frac` (a HARDWARE fraction: issued FLOPs or written bytes over time over peak) above 1 anywhere in a record, as
    (path, value) pairs.  Such a value means the timed kernels did not do the counted work (round 5: the soma volume counted peaks the
    engine had skipped, frac 1.89).  `frac_algorithmic` may exceed 1 (Winograd) and is not looked at."""
    bad = []
    if isinstance(rec, dict):
        for k, v in rec.items():
            here = "%s.%s" % (path, k) if path else k
            if k == "frac" and isinstance(v, (int, float)) and not isinstance(v, bool) and v > 1.0:
                bad.append((here, float(v)))
            else:
                bad += hardware_fracs_above_one(v, here)
    elif isinstance(rec, (list, tuple)):
        for i, v in enumerate(rec):
            bad += hardware_fracs_above_one(v, "%s[%d]" % (path, i))
    return bad


def emit(res, tag):
    """Full record -> stderr + gpurun_out/bench_full_<tag>.json (profiles/ keeps the judged copies); compact line -> stdout, LAST."""
    bad = hardware_fracs_above_one(res)
    if bad:                                              # loud, and on the line itself: tools/check_bench_line.py and the tests refuse it
        res["accounting_errors"] = ["%s = %.3f > 1" % b for b in bad]
        sys.stderr.write("[bench.py] ACCOUNTING ERROR: hardware fraction above 1: %s\n" % res["accounting_errors"])
    full = json.dumps(res)
    path = None
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "bench_full_%s.json" % tag)
        with open(path, "w") as f:
            f.write(full + "\n")
        path = os.path.relpath(path, ROOT)
    except OSError:
        path = None
    sys.stderr.write("[bench.py full record] " + full + "\n")
    sys.stderr.flush()
    sys.stdout.flush()
    print(compact_line(res, path), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 20; 200 for --workload backbone, whose step is < 1 ms)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed steps (default 5; 50 for --workload backbone)")
    ap.add_argument("--workload", default="detect", choices=["detect", "backbone", "prm", "prm-nuclei", "volume"])
    ap.add_argument("--vols-per-rank", type=int, default=0, help="volumes per rank per step (default 4 at every N; 8 = BASELINE configs[4]'s partition)")
    ap.add_argument("--full", action="store_true", help="detect / backbone workloads: after the headline also measure everything else - resident, "
                    "warm and sustained loops, rooflines, the N > 1 breakdown, the sub-records, CPU baselines - and write the full record")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="detect / backbone workloads: write what the last timed step returned "
                    "to DIR/<name>.npy (float32, at most 64 MB)")
    ap.add_argument("--interleaved", action="store_true", help="with --full: also time the one-stream begin(k+1) / finish(k) loop (N = 1)")
    ap.add_argument("--pipelined", action="store_true", help="with --full: also time the two-stream begin(k+1) / finish(k) loop (N = 1)")
    ap.add_argument("--stress-rois", action="store_true", help="RPN NMS threshold 1.0: every volume gives RPN_POST_NMS_TOP_N = 1000 RoIs to the box head")
    ap.add_argument("--prm-norm-stream", type=int, default=1, help="PRM workloads: 0 = norm convs queued on the tile's own stream instead of a second one (A/B)")
    ap.add_argument("--prm-rpn-logit-scale", type=float, default=0.25, help="PRM workloads: factor on the random-init RPN class logits of both nets (1.0 = the saturated sigmoids rounds 1-3 (nuclei) / 1-5 (soma) timed)")
    ap.add_argument("--prm-pipeline", type=int, default=0, help="PRM tile workloads: 1 = the two-tile software pipeline (m3d.prm.TilePipeline) instead of one prm_tile call per step (A/B: no faster)")
    ap.add_argument("--prm-f24-min", type=int, default=16, help="PRM workloads: smallest window that takes the F(2x4) strip family (A/B)")
    ap.add_argument("--prm-binarize-stream", type=int, default=1, help="PRM workloads: 0 = a tile's binarisation stage on the tile's stream instead of its own (where it runs beside the next tile's forward) (A/B)")
    ap.add_argument("--prm-backward-streams", type=int, default=1, help="PRM workloads: 2 = the peaks' back-propagation as two halves on two streams (A/B)")
    ap.add_argument("--prm-fused-prepare", type=int, default=1, help="PRM workloads: 0 = strip conv and the next layer's prepare as two launches (A/B)")
    ap.add_argument("--no-subrecords", action="store_true", help="with --full, default workload at N = 1: skip configs1_backbone / stress_rois / configs3_prm_soma / prm_nuclei_tile / volume_pipeline")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--dry", action="store_true", help="launcher + exchange rehearsal without a GPU (stub step)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--upload-at", default="end", choices=["mid", "end"], help="host-to-host loop: where the next step's pinned upload is issued (A/B, measured equal: 3.944 / 3.940 ms; see step_host)")
    args = ap.parse_args()
    if args.dump_outputs and (args.dry or args.workload not in ("detect", "backbone")):
        ap.error("--dump-outputs: the detect and backbone workloads only")
    if (args.interleaved or args.pipelined) and not args.full:
        ap.error("--interleaved / --pipelined are measured with --full")
    if args.steps is None:
        args.steps = 200 if args.workload == "backbone" else 20     # a timed region of ~0.1-0.2 s either way
    if args.warmup is None:
        args.warmup = 50 if args.workload == "backbone" else 5      # (3 left the first timed steps ~5 % slow: clocks / allocator still settling)

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        if not args.dry and args.backend == "nccl":
            import torch                                    # device_count() does not initialise the GPU
            have = torch.cuda.device_count()
            if have < args.gpus:
                raise SystemExit("bench.py --gpus %d: this node shows %d GPU(s); one rank per GPU over RCCL needs %d "
                                 "(--backend gloo rehearses more ranks than GPUs)" % (args.gpus, have, args.gpus))
        sys.exit(launch_ranks(args, sys.argv[1:]))          # children are created before anything here touches a GPU

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    dist = None
    if args.dry:
        if world > 1:
            import torch.distributed as dist
            dist.init_process_group("gloo", rank=rank, world_size=world)
        run_dry(args, rank, world, dist)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a GPU (the HIP path has no CPU fallback); --dry rehearses the launcher on CPU")
        torch.cuda.set_device(local_rank % torch.cuda.device_count())   # more ranks than GPUs only in the gloo rehearsal below
        if world > 1:
            import torch.distributed as dist
            if args.backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group("gloo", rank=rank, world_size=world)
        outputs = None
        if args.workload in ("prm", "prm-nuclei"):
            res = bench_prm(args, rank, world, dist)
        elif args.workload == "volume":
            res = bench_volume(args, rank, world, dist)
        else:
            res, outputs = bench_detect(args, rank, world, dist)
            if res is not None and args.full and args.workload == "detect" and world == 1 and not args.stress_rois and not args.no_subrecords:
                # the reference's DEFAULT mode is PRM_ON (both shipped YAMLs): its tiles and whole volumes ride on the default line
                import copy
                torch.cuda.empty_cache()
                for key, wl, steps, budget in (("configs3_prm_soma", "prm", 10, 18.0), ("prm_nuclei_tile", "prm-nuclei", 8, 18.0)):
                    sub = copy.copy(args)
                    sub.workload, sub.steps, sub.warmup = wl, steps, 3
                    try:
                        res[key] = condensed(bench_prm(sub, rank, world, dist, cpu_budget_s=budget))
                    except Exception as e:                   # a sub-record must not lose the headline
                        res[key] = {"error": "%s: %s" % (type(e).__name__, e)}
                    torch.cuda.empty_cache()
                # the nuclei tile of rounds 1-3 (saturated RPN sigmoids: 67 peaks whose maps are all 0 / 0, see prm_params) beside the repaired
                # one, so that the round-over-round trend reads off the line
                try:
                    sub = copy.copy(args)
                    sub.workload, sub.steps, sub.warmup, sub.prm_rpn_logit_scale, sub.no_cpu_baseline = "prm-nuclei", 10, 5, 1.0, True
                    old = bench_prm(sub, rank, world, dist)
                    if isinstance(res.get("prm_nuclei_tile"), dict) and old is not None:
                        res["prm_nuclei_tile"]["rounds_1_3_workload"] = {
                            "ms_per_step": old["ms_per_step"], "peaks_per_tile": old["config"]["peaks_per_tile"],
                            "instances_painted": old["config"]["instances_painted"],
                            "what": "the same code on the random init of rounds 1-3: every kept peak's RPN sigmoid is exactly 1.0f and its map 0 / 0 "
                                    "(round 5: the engine skips the back-propagation of such peaks)"}
                except Exception as e:
                    if isinstance(res.get("prm_nuclei_tile"), dict):
                        res["prm_nuclei_tile"]["rounds_1_3_workload"] = {"error": "%s: %s" % (type(e).__name__, e)}
                # configs[3] as rounds 1-5 ran it (soma RPN left saturated: a quarter of the 128 peaks dead and, since round 5, skipped)
                try:
                    sub = copy.copy(args)
                    sub.workload, sub.steps, sub.warmup, sub.prm_rpn_logit_scale, sub.no_cpu_baseline = "prm", 10, 3, 1.0, True
                    old = bench_prm(sub, rank, world, dist)
                    if isinstance(res.get("configs3_prm_soma"), dict) and old is not None:
                        res["configs3_prm_soma"]["rounds_1_5_workload"] = {
                            "ms_per_step": old["ms_per_step"], "peaks_per_tile": old["config"]["peaks_per_tile"],
                            "peaks_back_propagated": old["config"]["peaks_back_propagated"],
                            "what": "the same code on the soma net's random init as rounds 1-5 timed it (RPN sigmoids of the top peaks saturated)"}
                except Exception as e:
                    if isinstance(res.get("configs3_prm_soma"), dict):
                        res["configs3_prm_soma"]["rounds_1_5_workload"] = {"error": "%s: %s" % (type(e).__name__, e)}
                torch.cuda.empty_cache()
                try:
                    res["volume_pipeline"] = condensed(bench_volume(args, rank, world, dist, reps=2, cpu_budget_s=10.0))
                except Exception as e:
                    res["volume_pipeline"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if rank == 0 and res is not None:
            if args.dump_outputs:                        # after every measurement: nothing extra runs between the timed loops
                dump_outputs(args.dump_outputs, outputs)
            if args.full or args.workload not in ("detect", "backbone"):
                emit(res, "%s_n%d%s" % (args.workload, world, "_stress" if args.stress_rois else ""))
            else:                                            # a plain run: the headline line alone, no full record
                print(compact_line(res), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
