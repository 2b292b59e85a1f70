#!/usr/bin/env python3
"""Headline benchmark: genome fitness evaluations per second at 256x256, pop = 256, on 1/2/4/8 MI355X (BASELINE.json).

One "step" = one generation's fitness evaluation of the population through the drop-in path
(evolutionary_illusion_generator_amd.fitness.population_fitness: flatten genomes -> [rank 0 broadcasts the wire arrays] ->
CPPN render -> PredNet 21-step roll-out -> Lucas-Kanade -> score -> all-gather of the fitness scalars).  Workload =
BASELINE.json configs[2]: neat_configs/circles.txt (num_hidden 20, 3 outputs), colour, channels 3,48,96,192, Circles
structure, 256x256, ONE population of 256 genomes.  Data: seeded synthetic genomes and seeded synthetic PredNet weights
(the trained weights are external downloads and fix the size to 160x120).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--weak] [--dump-outputs DIR]
                    [--full [--no-cpu-baseline] [--no-roofline] [--no-parity] [--no-supplementary] [--strict-parity]]

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step returned to its caller -- the fitness
vector of the population, float64 -- as DIR/fitness.npy.  The workload is seeded, so two builds run with the same arguments
can be compared output for output.

--gpus N > 1 without a torch.distributed environment re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` (one rank per GPU, backend
nccl = RCCL); launched that way by the driver it just joins.  Either way it asserts WORLD_SIZE == N.
Scaling: the metric names ONE population of 256, so for N > 1 that population is sharded N ways ("scaling": "strong",
32 genomes per GPU at N = 8); --weak keeps --pop genomes PER GPU instead (supplementary).

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run does only what that line's headline needs: set
up, warm up, time the --steps generations, write --dump-outputs, print the line (`value`, `ms_per_step`, `config`,
`stage_ms_last_step`, `multi_gpu` for N > 1).

--full adds the untimed legs, AFTER the timed region and on rank 0 only (each can be left out with its --no-* option):
`roofline` (dominant kernel: the fused ConvLSTM 3x3 convolution on the fp32 MFMA pipe, timed live with HIP events on its
launch stream), `roofline_hbm` (the two HBM-side stages: CPPN render and the flow stencils), `cpu_baseline` (the CPU oracle's
path -- numpy CPPN + torch-CPU fp32 PredNet + C Lucas-Kanade + numpy scores -- on a bounded sample of >= 8 genomes at the
best of a small thread sweep), `parity_check` (genome 0 against the bit-exact C oracle; ALL genomes of the population
classified against the reference's element-wise order, oracle/classify.py), `supplementary` (the other BASELINE.json
configs, a few seconds each, never part of `value`) and, for N > 1, the N = 1 anchor `multi_gpu.n1_same_box_*`.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
PEAK_HBM_TBS = 8.0            # MI355X_MICROARCH.md: HBM3E
LSTM_KERNEL_TAG = "conv3x3_mfma<4, 16, 1"  # the dominant kernel's name in rocprofv3 output (EPI_LSTM = 1)
WINO4_KERNEL_TAG = "wino4_kernel<4, 1,"      # ... when the ConvLSTM chains run in their Winograd form: the F(4x4, 3x3) kernel (csrc/conv_wino4.h, the default; third template argument: the block shape -- wide at the headline shape)
N_STEPS_PREDNET = 21          # steps 1-20 + first extension (the 22nd step is never read on the population path)

SHAPES = {
    # name: (W, H, channels, c_dim, structure, n_hidden, n_outputs, default global pop, label)
    "headline": (256, 256, [3, 48, 96, 192], 3, 1, 20, 3, 256, "neat_configs/circles.txt colour"),
    "ref160": (160, 120, [3, 48, 96, 192], 3, 1, 20, 3, 50, "neat_configs/circles.txt colour"),
    # configs[0]: the reference's CPU-runnable plumbing case -- default.txt has num_inputs = 4, num_outputs = 6, num_hidden = 8 (:48-50); leaves
    # x, y, r, bias and the first output (build-defined: PyTorch-NEAT would assert), Free structure, 64x64 gray
    "c1": (64, 64, [1, 16, 32, 64], 1, 2, 8, 6, 10, "neat_configs/default.txt gray (4 inputs x, y, r, bias; first of 6 outputs)"),
    "c2": (160, 120, [1, 16, 32, 64], 1, 1, 20, 1, 50, "neat_configs/circles_bw.txt gray"),
    # the reference's other real size: `--size big` = 640x480 (generate_illusion.py:742-746); top-layer maps 80x60
    "ref640": (640, 480, [3, 48, 96, 192], 3, 1, 20, 3, 16, "neat_configs/circles.txt colour, --size big"),
    "c4": (256, 256, [3, 48, 96, 192], 3, 0, 8, 6, 512, "neat_configs/bands.txt colour (first 3 of 6 outputs)"),
    "c5": (512, 512, [3, 48, 96, 192], 3, 2, 20, 6, 1024, "neat_configs/free.txt colour (first 3 of 6 outputs)"),
}
SHAPE_INPUTS = {"c1": 4}  # CPPN leaves of a shape's NEAT config (default 2: x, y)
STRUCT_NAMES = ["Bands", "Circles", "Free", "CirclesFree"]
SCORE_NAMES = ["horizontal-symmetry", "rotation-symmetry", "swarm", "rotation-symmetry"]


def kernel_sources_sha():
    """Fingerprint of everything that is compiled into libeigen_hip.so: a PMC summary is only valid for the build it was
    taken on (profiles/pmc_summary_latest.json carries the same hash, written by scripts/summarize_pmc.py)."""
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "evolutionary_illusion_generator_amd", "csrc")
    for f in sorted(x for x in os.listdir(csrc) if x.endswith((".h", ".hip"))) + [os.path.join(ROOT, "include", "eigen_engine.h")]:
        p = f if os.path.isabs(f) else os.path.join(csrc, f)
        h.update(os.path.basename(p).encode())
        h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def git_head():
    """Commit the running build was made at: git here, BUILD_INFO.json (written by __graft_entry__.build()) on the GPU box."""
    try:
        return subprocess.check_output(["git", "-C", ROOT, "describe", "--always", "--dirty"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        pass
    try:
        return json.load(open(os.path.join(ROOT, "evolutionary_illusion_generator_amd", "BUILD_INFO.json")))["commit"]
    except Exception:
        return None


def _whole_host_worker(idx, threads, cpus, shape_name, window_s, ready, go, q):
    """One worker process of the whole-host CPU figure: its own torch-CPU PredNet on `threads` threads (pinned to `cpus`), the full
    oracle path on genomes of the same population for `window_s` seconds after the common start signal."""
    try:
        if cpus:
            os.sched_setaffinity(0, cpus)
    except OSError:
        pass
    os.environ["OMP_NUM_THREADS"] = str(threads)
    import numpy as np
    import torch
    torch.set_num_threads(threads)
    import oracle
    from oracle import pipeline, scores
    from oracle.prednet_torch import PredNetTorch
    from evolutionary_illusion_generator_amd import grids
    oracle.set_threads(1)
    W, H, CHANNELS, C_DIM, STRUCTURE = SHAPES[shape_name][:5]
    cfg, population, wts = make_workload(shape_name, 64)
    grid = grids.create_grid(STRUCTURE, W, H, 10)
    net = PredNetTorch(wts, CHANNELS, W, H)
    img = pipeline.render_chw(population[0][1], cfg, grid, C_DIM, W, H)
    net.rollout(img[None], n_repeat=1, n_ext=0)
    ready.put(idx)
    go.wait()
    t0, done, t_last = time.time(), 0, time.time()
    while time.time() - t0 < window_s:
        g = population[(idx * 7 + done) % len(population)][1]
        img = pipeline.render_chw(g, cfg, grid, C_DIM, W, H)
        frames, _ = net.rollout(img[None], n_repeat=20, n_ext=1)
        v = oracle.lucas_kanade(frames[0, 19], frames[0, 20])
        scores.fitness_from_vectors(STRUCTURE, v.astype(np.float64), W, H)
        done += 1
        t_last = time.time()
    q.put((idx, done, t_last - t0))


def _cgroup_cpu_limit():
    """CPUs' worth of time the container may use (cgroup v2 cpu.max / v1 cfs quota), or None when unlimited / unknown."""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if quota == "max" else float(quota) / float(period)
    except Exception:  # noqa: BLE001
        pass
    try:
        quota = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        period = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if quota <= 0 else quota / period
    except Exception:  # noqa: BLE001
        return None


def cpu_whole_host(shape_name, threads, window_s=12.0, max_workers=16, timeout_s=90.0):
    """floor(usable_cpus / threads) worker processes (at most max_workers), each evaluating independent genomes of the same
    population through the full oracle path at the same time for `window_s` seconds: genome evals/s of the BOX, not of one
    process.  usable_cpus = the affinity mask, or the cgroup CPU quota where one is set."""
    import multiprocessing as mp
    try:
        allowed = sorted(os.sched_getaffinity(0))
    except AttributeError:
        allowed = list(range(os.cpu_count() or 1))
    quota = _cgroup_cpu_limit()
    usable = len(allowed) if quota is None else max(1, min(len(allowed), int(quota)))
    workers = max(1, min(max_workers, usable // threads))
    ctx = mp.get_context("spawn")
    ready, q, go = ctx.Queue(), ctx.Queue(), ctx.Event()
    procs = [ctx.Process(target=_whole_host_worker, args=(i, threads, allowed[i * threads:(i + 1) * threads], shape_name, window_s, ready, go, q)) for i in range(workers)]
    for p in procs:
        p.start()
    try:
        for _ in procs:
            ready.get(timeout=timeout_s)
        go.set()
        res = [q.get(timeout=timeout_s + window_s) for _ in procs]
    finally:
        go.set()
        for p in procs:
            p.join(timeout=10)
            if p.is_alive():
                p.kill()
    done = sum(r[1] for r in res)
    span = max(max(r[2] for r in res), window_s)
    return {"value": done / span, "unit": "genome evals/s", "workers": workers, "threads_per_worker": threads,
            "cores": workers * threads, "genomes": done, "seconds": span, "host_cpus": len(allowed), "cgroup_cpu_quota": quota,
            "sample": "%d processes x %d threads (pinned to disjoint CPU blocks), each evaluating genomes for %.0f s, full oracle path, all at once" % (workers, threads, window_s)}


def cpu_baseline(cfg, pop, wts, grid, shape, min_genomes=8, seconds_budget=20.0, flops_per_genome=None, shape_name="headline"):
    """The oracle's CPU path on a bounded sample of the same workload (rank 0, N = 1 only), with a per-stage split.
    The PredNet leg (99 % of it) is torch-CPU / oneDNN; its thread count is the best of a small sweep on 2 genomes each
    (batch-1 convolutions on a 256-CPU host are slower on 128 threads than on 32: VERDICT r2), and the >= 8-genome measurement
    runs at that setting.  Two denominators: `value` = ONE process at its best thread count; `whole_host` =
    as many such processes as the host has CPUs for (cap 16), independent genomes, all at once."""
    import numpy as np
    import torch
    from oracle import pipeline, scores
    from oracle.prednet_torch import PredNetTorch
    import oracle
    W, H, CHANNELS, C_DIM, STRUCTURE = shape[:5]
    net = PredNetTorch(wts, CHANNELS, W, H)
    default_threads = torch.get_num_threads()
    ncpu = os.cpu_count() or 1
    imgs = [pipeline.render_chw(pop[i][1], cfg, grid, C_DIM, W, H) for i in range(2)]
    net.rollout(imgs[0][None], n_repeat=1, n_ext=0)  # primitive creation is not part of anyone's measurement
    sweep = {}
    for th in sorted({t for t in (4, 8, 16, 32) if t <= ncpu} or {default_threads}):
        torch.set_num_threads(th)
        t0 = time.time()
        for im in imgs:
            net.rollout(im[None], n_repeat=20, n_ext=1)
        sweep[th] = (time.time() - t0) / len(imgs)
        if sweep[th] > 3.0 * min(sweep.values()):
            break  # clearly past the optimum: do not spend the budget there
    threads = min(sweep, key=sweep.get)
    torch.set_num_threads(threads)
    done, t0 = 0, time.time()
    fits, split = [], {"render_s": 0.0, "prednet_s": 0.0, "flow_s": 0.0, "score_s": 0.0}
    while done < len(pop) and (done < min_genomes or time.time() - t0 < seconds_budget):
        g = pop[done][1]
        ta = time.time()
        img = pipeline.render_chw(g, cfg, grid, C_DIM, W, H)
        tb = time.time()
        frames, _ = net.rollout(img[None], n_repeat=20, n_ext=1)
        tc = time.time()
        v = oracle.lucas_kanade(frames[0, 19], frames[0, 20])
        td = time.time()
        fits.append(scores.fitness_from_vectors(STRUCTURE, v.astype(np.float64), W, H))
        te = time.time()
        for k, d in zip(split, (tb - ta, tc - tb, td - tc, te - td)):
            split[k] += d
        done += 1
    dt = time.time() - t0
    torch.set_num_threads(default_threads)
    # a shared host can slow the timed loop down (seen: 2.1 s per genome in the loop right after 0.76 s in the sweep at the same
    # thread count): the reported rate is the FASTER of the two estimates, so that gpu_over_cpu is never flattered by a noisy box
    other = (split["render_s"] + split["flow_s"] + split["score_s"]) / done
    rate_loop, rate_sweep = done / dt, 1.0 / (sweep[threads] + other)
    out = {"value": max(rate_loop, rate_sweep), "value_timed_loop": rate_loop, "value_from_thread_sweep": rate_sweep,
           "unit": "genome evals/s", "cores": threads, "kind": "port",
           "host_cpus": ncpu, "genomes": done, "seconds": dt,
           "per_stage_s_per_genome": {k: v / done for k, v in split.items()},
           "thread_sweep_prednet_s_per_genome": {str(k): round(v, 3) for k, v in sweep.items()},
           "sample": "%d genomes of the same %dx%d population, full path (numpy float64 CPPN 1 thread, torch-CPU/oneDNN fp32 "
                     "PredNet 21 steps on %d threads = best of the sweep %s, C Lucas-Kanade 1 thread, numpy scores), %.1f s"
                     % (done, W, H, threads, sorted(sweep), dt)}
    if flops_per_genome:
        out["prednet_gflops"] = flops_per_genome / min(split["prednet_s"] / done, sweep[threads]) / 1e9  # the reference's 9-tap formulation
    try:
        wh = cpu_whole_host(shape_name, threads)
        if flops_per_genome:
            wh["prednet_gflops"] = flops_per_genome * wh["value"] / 1e9  # (whole path in the denominator: PredNet is 99 % of it)
        out["whole_host"] = wh
    except Exception as e:  # noqa: BLE001  (a failed worker pool must not cost the headline line)
        out["whole_host"] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out, fits


def classify_population(eng, fitness_mod, genomes, cfg, wts, shape, n_max=256, batch=8, n_cpu_control=12, n_c_reference=4):
    """north_star's "within 1e-4 relative" as a property checked for EVERY genome of the benchmark population (untimed leg):
    the HIP path's frames / vectors / fitness against the reference's element-wise order (chainer ConvLSTM: separate
    convolution tensors added left to right, un-fused gate products, sigmoid = tanh(x/2)/2 + 1/2, plain unpool -> 9-tap)
    with im2col + rocBLAS matmul convolutions on the GPU; Lucas-Kanade and scores of that side by the C / numpy oracle.
    oracle/classify.py: a genome outside 1e-4 must be reproduced by +-1 byte flips applied to the HIP path's own frames.

    CONTROL: the same classification between two NON-HIP implementations of the reference's order that differ
    only in the summation order inside a convolution -- (A) im2col + rocBLAS matmul vs (B) the library convolution (MIOpen picks the
    algorithm, as cuDNN does on the reference's `gpu=0` path, generate_illusion.py:485) on all genomes, and (A) vs (C) torch-CPU /
    oneDNN (the reference's CPU path, north_star) on the first n_cpu_control genomes.  If two reference-order implementations disagree
    with each other as often as HIP disagrees with one of them, the deviations are the conditioning of the fitness function."""
    import numpy as np
    import torch
    from evolutionary_illusion_generator_amd import genome as genome_mod
    from oracle import classify
    from oracle.prednet_torch import PredNetTorch
    W, H, CHANNELS, C_DIM, STRUCTURE = shape[:5]
    n = min(n_max, len(genomes), eng.max_batch)
    t0 = time.time()
    gb = genome_mod.GenomeBatch(genomes[:n], cfg, C_DIM, n_leaves=len(cfg.genome_config.input_keys))
    d_img = torch.empty((n, C_DIM, H, W), dtype=torch.uint8, device="cuda")
    eng.render_cppn(gb, d_img)
    fit, vecs = eng.eval_images(d_img, n, STRUCTURE, pairing=0)
    d_fr = torch.empty((n, 2, C_DIM, H, W), dtype=torch.uint8, device="cuda")
    eng.prednet_rollout(d_img, n, 21, 19, d_fr)
    torch.cuda.synchronize()
    imgs, frames = d_img.cpu().numpy(), d_fr.cpu().numpy()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    net = PredNetTorch(wts, CHANNELS, W, H, device="cuda", conv="matmul", order="chainer")
    side_a = classify.rollout_side(STRUCTURE, W, H, imgs, net, batch=batch)
    summ, _ = classify.population_report(STRUCTURE, W, H, imgs, frames, vecs, fit, None, other=side_a)
    summ["against"] = "reference element-wise order (chainer ConvLSTM.__call__), im2col + rocBLAS fp32 matmul on the GPU; C Lucas-Kanade + numpy scores"
    summ["seconds"] = time.time() - t0
    t1 = time.time()
    try:
        net_b = PredNetTorch(wts, CHANNELS, W, H, device="cuda", conv="library", order="chainer")
        side_b = classify.rollout_side(STRUCTURE, W, H, imgs, net_b, batch=batch)
        ctl = classify.control_report(STRUCTURE, W, H, side_a, side_b, "reference order, im2col + rocBLAS matmul (GPU)", "reference order, MIOpen library convolution (GPU)")
        ctl["control_seconds"] = time.time() - t1
        summ["control"] = ctl
        # HIP against the second reference-order implementation as well: the 1e-4 count must not depend on which one is asked
        s_b, _ = classify.population_report(STRUCTURE, W, H, imgs, frames, vecs, fit, None, other=side_b)
        summ["vs_second_reference_order_implementation"] = {k: s_b[k] for k in ("within_1e-4", "outside_1e-4", "outside_1e-4_unexplained", "byte_flip_rate", "identical_frames")}
    except Exception as e:  # noqa: BLE001
        summ["control"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if n_cpu_control:
        t2 = time.time()
        m = min(n, n_cpu_control)
        threads0 = torch.get_num_threads()
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        net_c = PredNetTorch(wts, CHANNELS, W, H, order="chainer")
        side_c = classify.rollout_side(STRUCTURE, W, H, imgs[:m], net_c, batch=1)
        torch.set_num_threads(threads0)
        cut = lambda sd: (sd[0][:m], sd[1][:m], sd[2][:m])
        ctl = classify.control_report(STRUCTURE, W, H, cut(side_a), side_c, "reference order, im2col + rocBLAS matmul (GPU)", "reference order, torch-CPU / oneDNN")
        s_c, _ = classify.population_report(STRUCTURE, W, H, imgs[:m], frames[:m], vecs[:m], fit[:m], None, other=side_c)
        ctl["hip_vs_cpu_reference_order"] = {k: s_c[k] for k in ("genomes", "within_1e-4", "outside_1e-4", "outside_1e-4_unexplained", "byte_flip_rate", "identical_frames")}
        ctl["control_seconds"] = time.time() - t2
        summ["control_cpu"] = ctl
    if n_c_reference:
        # north_star's bar against the TORCH-FREE C statement of the reference's element-wise order (oracle.PredNetC, host-independent: plain loops, one
        # fp32 fma chain per output in (channel, ky, kx) order), on the first genomes that score non-zero (the test of the same name asserts it)
        import oracle
        t3 = time.time()
        nz = [i for i in range(n) if fit[i] != 0][:n_c_reference]
        if nz:
            s_r, _ = classify.population_report(STRUCTURE, W, H, imgs[nz], frames[nz], [vecs[i] for i in nz], np.asarray(fit)[nz], oracle.PredNetC(wts, CHANNELS, W, H, order="chainer"), batch=1)
            summ["vs_c_reference_order"] = dict({k: s_r[k] for k in ("genomes", "within_1e-4", "outside_1e-4", "outside_1e-4_unexplained", "byte_flip_rate", "max_byte_diff",
                                                                       "identical_frames", "max_rel", "nonzero_both")},
                                                genome_indices=nz, seconds=time.time() - t3,
                                                against="reference element-wise order, torch-free C statement (oracle/eig_oracle.c order=chainer), CPU")
    return summ, fit


def respawn_under_torchrun(n):
    """`python bench.py --gpus N` from a plain shell: become N ranks (one per GPU) under torch.distributed.run."""
    import torch
    have = torch.cuda.device_count()
    if have < n:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible" % (n, have))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # the host driver only supports dmabuf IPC (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def conv_roofline(eng, fitness_mod, workload, nb):
    """Per-launch HIP-event timing of every conv kernel of one more roll-out pass (events on the launch stream) ->
    (rows, dominant-kernel summary, all-conv summary)."""
    STRUCTURE, genomes, wts, cfg, W, H, CHANNELS, C_DIM, max_batch = workload
    eng.conv_profile(True, reset=True)
    fitness_mod.evaluate_population(STRUCTURE, genomes[:nb], wts, cfg, W, H, CHANNELS, c_dim=C_DIM, gradient=1, max_batch=max_batch)
    rows = eng.conv_profile(False, reset=True)
    all_fl = sum(r["flops_per_image"] * nb * r["launches"] for r in rows)
    all_ms = sum(r["ms"] for r in rows)
    allc = {"achieved": all_fl / (all_ms * 1e-3) / 1e12, "frac": all_fl / (all_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
            "total_ms": all_ms, "launches": sum(r["launches"] for r in rows)}
    return rows, all_fl, allc


def survey_8d_convlstm_macs(channels, W, H, l):
    """multiply-adds of ConvLSTM_l per genome and PredNet step in the REFERENCE's formulation -- 3x3 taps
    on every source (E_l: 2 C_l channels, the unpooled R_{l+1}: C_{l+1}, h_l: C_l), 4 gates x C_l outputs at H_l x W_l."""
    C = channels[l]
    cin = 2 * C + C + (channels[l + 1] if l + 1 < len(channels) else 0)
    return 4.0 * C * (H >> l) * (W >> l) * cin * 9


def convlstm_algorithmic_bytes(channels, W, H, l):
    """Algorithmic HBM bytes of one ConvLSTM_l launch PER GENOME: every source once (E_l, h_l at H_l x W_l, R_{l+1} at half of it), the cell
    state in and out, h out; fp32."""
    C, px = channels[l], (H >> l) * (W >> l)
    src = (2 * C + C) * px + (channels[l + 1] * (px // 4) if l + 1 < len(channels) else 0)
    return 4.0 * (src + 2 * C * px + C * px)


def make_workload(shape_name, global_pop):
    from evolutionary_illusion_generator_amd import synth, weights
    W, H, CHANNELS, C_DIM, STRUCTURE, n_hidden, n_outputs, _, _ = SHAPES[shape_name]
    cfg = synth.make_config(SHAPE_INPUTS.get(shape_name, 2), n_outputs)
    population = synth.make_population(global_pop, cfg, seed=0, num_hidden=n_hidden)  # identical on every rank (seeded)
    wts = weights.synthetic_prednet_weights(CHANNELS, W, H, seed=0)
    return cfg, population, wts


def supplementary_shape(name, pop, steps, warmup=1, report_memory=False):
    """One of the other BASELINE.json configurations, single GPU, a few seconds: evals/s through the same drop-in path and the
    all-conv roofline fraction of one profiled pass.  Never part of `value`."""
    import torch
    from evolutionary_illusion_generator_amd import fitness
    W, H, CHANNELS, C_DIM, STRUCTURE, _, _, default_pop, label = SHAPES[name]
    cfg, population, wts = make_workload(name, pop)
    genomes = [g for _, g in population]
    max_batch = min(pop, 256)
    eng = fitness.get_engine(wts, W, H, CHANNELS, max_batch=max_batch)
    run = lambda: fitness.population_fitness(STRUCTURE, genomes, wts, cfg, W, H, CHANNELS, c_dim=C_DIM, gradient=1, max_batch=max_batch)
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fit = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nb = min(max_batch, pop)
    _, all_fl, allc = conv_roofline(eng, fitness, (STRUCTURE, genomes, wts, cfg, W, H, CHANNELS, C_DIM, max_batch), nb)
    flops_ref = eng.flops_per_step() * N_STEPS_PREDNET
    out = {"workload": "%s pop=%d, %dx%d, PredNet %s, %s score%s" % (label, pop, W, H, ",".join(map(str, CHANNELS)), SCORE_NAMES[STRUCTURE],
                                                                    "" if pop == default_pop else " (config pop %d: device-batch sample)" % default_pop),
           "value": pop * steps / dt, "unit": "genome evals/s", "steps": steps, "ms_per_step": 1e3 * dt / steps, "device_batch": max_batch,
           "nonzero_fitness": int((fit != 0).sum()),
           "all_conv_frac": allc["frac"], "all_conv_tflops": allc["achieved"], "conv_launches": allc["launches"],
           "tflops_on_survey_8d_flops": flops_ref * pop * steps / dt / 1e12}
    if report_memory:
        free, total = torch.cuda.mem_get_info()
        out["device_memory_in_use_gb"] = (total - free) / 1e9   # everything this process holds on the device while the engine of this shape exists
        out["device_batches"] = -(-pop // max_batch)
    return out


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy (float64 stays float64, anything else becomes float32)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        np.save(os.path.join(out_dir, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pop", type=int, default=None, help="population size (global; per GPU with --weak). Default: the shape's (256)")
    ap.add_argument("--weak", action="store_true", help="supplementary: keep --pop genomes PER GPU (weak scaling) instead of sharding ONE population")
    ap.add_argument("--shape", default="headline", choices=sorted(SHAPES),
                    help="headline: 256x256 colour pop 256 (BASELINE.json metric, configs[2]); ref160: the reference's own default "
                         "160x120 colour, pop 50 (the only published datum: 0.80 evals/s on a Colab GPU, BASELINE.md); "
                         "c1: configs[0] default.txt 64x64 gray pop 10 (4 CPPN inputs); c2: configs[1] circles_bw 160x120 gray (channels 1,16,32,64) pop 50; ref640: the reference's --size big, 640x480 colour pop 16; c4: configs[3] bands.txt (8 hidden, "
                         "6 outputs) 256x256 colour Bands pop 512; c5: configs[4] free.txt 512x512 colour Free structure pop 1024")
    ap.add_argument("--flow", default="lk", choices=["lk", "farneback"],
                    help="supplementary: 'farneback' swaps the reference's Lucas-Kanade call for the dense Farneback option (no CPU leg)")
    ap.add_argument("--source", default=None, choices=["rank0", "replicated"], help="multi-rank genome source (fitness.GENOME_SOURCE)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run the untimed legs: roofline, CPU baseline, parity, supplementary shapes, "
                         "the N = 1 anchor of a multi-GPU run (a plain run only times the steps and prints the headline line)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline leg")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline legs (one profiled roll-out pass)")
    ap.add_argument("--no-parity", action="store_true", help="with --full: skip the untimed parity legs (C-oracle spot check, whole-population classification)")
    ap.add_argument("--no-supplementary", action="store_true", help="with --full: skip the untimed supplementary block (ref160, c2, c4, c5 at a device-batch sample)")
    ap.add_argument("--strict-parity", action="store_true", help="with --full: exit with status 3 when the parity legs flag a failure (parity_fail)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the population's fitness, float64) as DIR/fitness.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (the timed region is --steps generations)")
    if args.strict_parity and not (args.full and not args.no_parity):
        ap.error("--strict-parity needs the parity legs: add --full (without --no-parity)")
    if not args.full:
        args.no_cpu_baseline = args.no_roofline = args.no_parity = args.no_supplementary = True
    # RCCL / device-tensor sharing across processes needs dmabuf IPC on these hosts; must be in the environment BEFORE the HIP
    # runtime initialises, whoever launched this process (the respawn path below, the driver's own torchrun, a plain shell)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d but WORLD_SIZE=%d: launch with --nproc-per-node %d" % (args.gpus, world, args.gpus))

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    # EIGEN_BENCH_BACKEND=gloo (tests only): the N-rank control flow of this file on a box with FEWER GPUs than ranks -- the ranks
    # share the visible devices and gloo carries the collectives; RCCL refuses two ranks on one device.  Never a measurement.
    backend = os.environ.get("EIGEN_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank % torch.cuda.device_count() if backend != "nccl" else local_rank)
    import torch.distributed as dist
    # EIGEN_DIST_SINGLE=1 (tests): take the whole multi-rank path -- RCCL group, broadcast, all-gather, per-rank report, leaving the
    # group before rank 0's untimed legs -- in a group of ONE rank, which is all a single-GPU box can run of it
    use_dist = world > 1 or os.environ.get("EIGEN_DIST_SINGLE") == "1"
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1 and "MASTER_PORT" not in os.environ:
            s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); os.environ["MASTER_PORT"] = str(s_.getsockname()[1]); s_.close()
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        assert dist.get_backend() == backend and dist.get_world_size() == args.gpus

    shape = SHAPES[args.shape]
    W, H, CHANNELS, C_DIM, STRUCTURE, n_hidden, n_outputs, default_pop, label = shape
    supplementary = args.shape != "headline" or args.flow != "lk" or args.weak
    if supplementary:
        args.no_cpu_baseline = args.no_parity = args.no_supplementary = True  # supplementary numbers: no CPU / parity legs
    pop_arg = args.pop or default_pop
    if pop_arg != default_pop:
        args.no_supplementary = True
    global_pop = pop_arg * world if args.weak else pop_arg
    per_rank = -(-global_pop // world)
    max_batch = min(per_rank, 256)
    timed_device_batch = max_batch

    from evolutionary_illusion_generator_amd import fitness, grids
    if args.flow != "lk":
        fitness.FLOW_METHOD = args.flow
    cfg, population, wts = make_workload(args.shape, global_pop)
    genomes = [g for _, g in population]
    eng = fitness.get_engine(wts, W, H, CHANNELS, max_batch=max_batch, **({} if args.flow == "lk" else {"flow": args.flow}))

    def step():
        return fitness.population_fitness(STRUCTURE, genomes, wts, cfg, W, H, CHANNELS, c_dim=C_DIM, gradient=1,
                                          max_batch=max_batch, source=args.source)

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    shard_stats = []
    for _ in range(args.steps):
        fit = step()
        if use_dist:
            shard_stats.append(dict(fitness.LAST_SHARD_STATS))
    fence()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"fitness": fit})
    multi = None
    if use_dist:
        tmax = torch.tensor([dt], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
        # what every rank spent inside its shard's evaluate() (rode in the fitness all-gather itself) and what the collective cost here:
        # a straggling GPU shows as max >> min, a slow collective as collective_ms; averaged over the timed steps
        # proof that the collective saw N ranks: an all-gather of (rank, local device index) on the same backend
        ids = torch.tensor([rank, torch.cuda.current_device()], dtype=torch.int64, device="cuda" if backend == "nccl" else "cpu")
        seen = torch.empty(2 * world, dtype=torch.int64, device=ids.device)
        dist.all_gather_into_tensor(seen, ids)
        seen = seen.cpu().numpy().reshape(world, 2)
        # every rank must run the same canonical arithmetic (EIGEN_WINOGRAD selects it): gathered beside the ranks
        # (the EFFECTIVE mask as the library resolved it -- EIGEN_WINO_FUSEUP=0 clears bit 24 and moves the ConvLSTMs below the top to another order: ADVICE r5)
        from evolutionary_illusion_generator_amd import engine as engine_mod
        mk = torch.tensor([int(engine_mod.load_library().eigen_winograd_mask()) & 0xFFFFFFFF], dtype=torch.int64, device=ids.device)
        masks = torch.empty(world, dtype=torch.int64, device=ids.device)
        dist.all_gather_into_tensor(masks, mk)
        masks = [int(x) for x in masks.cpu().numpy()]
        if len(set(masks)) != 1:
            raise SystemExit("bench.py: the ranks run different EIGEN_WINOGRAD / EIGEN_WINO_FUSEUP settings (%s): their fitness values are not comparable" % ["0x%08X" % m for m in masks])
        try:
            rccl_version = ".".join(str(v) for v in torch.cuda.nccl.version()) if backend == "nccl" else None
        except Exception:  # noqa: BLE001
            rccl_version = None
        loc = np.asarray([s_["local_ms"] for s_ in shard_stats], dtype=np.float64).mean(axis=0)
        multi = {"backend": backend, "rccl_version": rccl_version, "world_size": dist.get_world_size(), "ranks_seen": [int(x) for x in seen[:, 0]],
                 "devices_seen": [int(x) for x in seen[:, 1]], "hsa_ipc_mode_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"),
                 "winograd_mask_all_ranks": "0x%08X" % masks[0],
                 "per_rank_device_ms": [round(float(x), 3) for x in loc], "device_ms_max": float(loc.max()), "device_ms_min": float(loc.min()),
                 "collective_ms_rank0": float(np.mean([s_["collective_ms"] for s_ in shard_stats])),
                 "note": "per-rank evaluate() wall time of its shard (flatten/slice + render + roll-out + flow + score + D2H), mean over the timed "
                         "steps; collective_ms = rank 0's all-gather incl. its wait for the slowest rank"}
        # Everything below is rank 0's untimed reporting: leave the process group TOGETHER now, so that no rank sits in a
        # collective (with its watchdog) while rank 0 profiles -- the other ranks are done.
        dist.barrier()
        dist.destroy_process_group()
        if rank != 0:
            return
        if world > 1 and args.full:
            # the SCALE line carries its own N = 1 anchor -- rank 0, now alone, evaluates the WHOLE population on its one GPU (one warm-up
            # + one timed generation, untimed by the driver), so that a mismatch with the N = 1 BENCH record is visible in one record
            fitness.clear_engines()
            torch.cuda.empty_cache()
            mb1 = min(global_pop, 256)
            run1 = lambda: fitness.population_fitness(STRUCTURE, genomes, wts, cfg, W, H, CHANNELS, c_dim=C_DIM, gradient=1, max_batch=mb1)
            run1()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            fit1 = run1()
            torch.cuda.synchronize()
            dt1 = time.perf_counter() - t1
            multi["n1_same_box_evals_s"] = global_pop / dt1
            multi["n1_same_box_ms_per_step"] = 1e3 * dt1
            multi["n1_same_box_fitness_equal"] = bool(np.array_equal(np.asarray(fit1), np.asarray(fit)))
            eng = fitness.get_engine(wts, W, H, CHANNELS, max_batch=mb1, **({} if args.flow == "lk" else {"flow": args.flow}))
            max_batch = mb1   # (rank 0's untimed legs below run at the single-GPU device batch; config.device_batch stays the timed region's)
    stage = eng.timings()

    out = {
        "metric": "genome fitness evals/sec at %dx%d, pop=%d" % (W, H, pop_arg) + (" per GPU" if args.weak else ""),
        "value": global_pop * args.steps / dt,
        "unit": "genome evals/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1000.0 * dt / args.steps,
        "higher_is_better": True, "scaling": "weak" if args.weak else "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": "%s pop=%d%s, %dx%d, PredNet %s, 21 steps, %s + %s score" % (
                       label, pop_arg, "/GPU" if args.weak else "", W, H, ",".join(map(str, CHANNELS)),
                       {"lk": "LK", "farneback": "Farneback dense flow"}[args.flow], SCORE_NAMES[STRUCTURE]),
                   "global_pop": global_pop, "genomes_per_gpu": per_rank, "device_batch": timed_device_batch, "image": [W, H],
                   "channels": CHANNELS, "structure": STRUCT_NAMES[STRUCTURE],
                   "parallelism": "pop-shard x%d (%s) + all-gather(fitness f64, %s)" % (
                       world, "genome wire arrays broadcast from rank 0" if (args.source or fitness.GENOME_SOURCE) == "rank0" else "replicated seeded populations",
                       ("RCCL" if backend == "nccl" else backend + " (TEST backend, not a measurement)") if use_dist else "single process")},
        "stage_ms_last_step": {k: round(v, 3) for k, v in stage.items() if k.endswith("_ms") and k != "conv_ms"},
        "nonzero_fitness": int((fit != 0).sum()),
        "commit": git_head(), "kernel_sources_sha": kernel_sources_sha(),
    }
    if multi:
        out["multi_gpu"] = multi

    if not args.no_roofline:
        nb = min(max_batch, len(genomes))
        rows, all_fl, allc = conv_roofline(eng, fitness, (STRUCTURE, genomes, wts, cfg, W, H, CHANNELS, C_DIM, max_batch), nb)
        lstm = [r for r in rows if r["epi"] == "lstm" and r["NI"] == 4]
        fl = sum(r["flops_per_image"] * nb * r["launches"] for r in lstm)
        ms = sum(r["ms"] for r in lstm)
        n_l = sum(r["launches"] for r in lstm)
        ach = fl / (ms * 1e-3) / 1e12
        # HBM traffic per launch of the same kernel: rocprofv3 --pmc passes cannot be collected from inside this process
        # (separate runs of this command: scripts/pmc_passes.sh + scripts/summarize_pmc.py; FETCH_SIZE doubled as
        # MI355X_MICROARCH.md prescribes for 16 B/lane reads).  The summary is stamped with the hash of the kernel sources
        # it was taken on; a summary of another build is NOT reported (traffic = null).
        traffic, traffic_commit, traffic_note, mfma_insts = None, None, None, None
        try:
            pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_summary_latest.json")))
            traffic_commit = pm.get("commit")
            if pm.get("kernel_sources_sha") != out["kernel_sources_sha"]:
                traffic_note = "profiles/pmc_summary_latest.json was taken on kernel sources %s, this build is %s: not reported" % (
                    pm.get("kernel_sources_sha"), out["kernel_sources_sha"])
            elif pm.get("pop") != nb:
                traffic_note = "PMC summary is for a device batch of %s genomes, this run uses %d: not reported" % (pm.get("pop"), nb)
            else:
                tags = (WINO4_KERNEL_TAG,) if any(r.get("wino") for r in lstm) else (LSTM_KERNEL_TAG,)
                for tag in tags:   # (the first tag the summary holds: the kernel that ran the ConvLSTMs of that build)
                    hit = [kv for kname, kv in pm["kernels"].items() if tag in kname]
                    if hit:
                        traffic = hit[0].get("hbm_read_bytes_per_launch", 0.0) + hit[0].get("hbm_write_bytes_per_launch", 0.0)
                        if hit[0].get("counters", {}).get("SQ_INSTS_MFMA") and hit[0].get("calls"):
                            mfma_insts = hit[0]["counters"]["SQ_INSTS_MFMA"] / hit[0]["calls"]
                        break
        except Exception as e:  # noqa: BLE001
            traffic_note = "no PMC summary: %s" % e
        flops_step = eng.flops_per_step()
        wino_rows = [r for r in lstm if r.get("wino")]
        secs = ms * 1e-3
        # the reference's formulation of the SAME launches -- 9 taps on every source, every step (the step-0
        # launch counted like any other).  Computed here from the layer shapes, not from what the kernel executes.
        s8d_layer = {l_: survey_8d_convlstm_macs(CHANNELS, W, H, l_) for l_ in sorted({r["layer"] for r in lstm})}
        s8d_fl = sum(2.0 * s8d_layer[r["layer"]] * nb * r["launches"] for r in lstm)
        alg_bytes = {l_: convlstm_algorithmic_bytes(CHANNELS, W, H, l_) * nb for l_ in s8d_layer}
        launches_l = {l_: sum(r["launches"] for r in lstm if r["layer"] == l_) for l_ in s8d_layer}
        alg_bytes_avg = sum(alg_bytes[l_] * launches_l[l_] for l_ in alg_bytes) / max(n_l, 1)
        from evolutionary_illusion_generator_amd import engine as engine_mod
        wmask = int(engine_mod.load_library().eigen_winograd_mask()) & 0xFFFFFFFF   # (the effective mask, as the library resolved it)
        out["roofline"] = {"bound": "mfma", "kernel": ("wino4_kernel<4,EPI_LSTM> (ConvLSTM, E / unpooled R / h chains as Winograd F(4x4,3x3): 36 multiply-adds per channel and 4x4 outputs where the direct form needs 144, fused gates, v_mfma_f32_16x16x4_f32)"
                                                       if wino_rows else "conv3x3_mfma<4,16,EPI_LSTM> (fused ConvLSTM gates, v_mfma_f32_16x16x4_f32)"),
                           "winograd_mask": "0x%08X" % wmask,
                           "winograd_layers": sorted({r["layer"] for r in wino_rows}),
                           # `achieved` / `frac`: the multiply-adds the kernel EXECUTES (= SQ_INSTS_MFMA x 2048 FLOP, checkable below) over its HIP-event time
                           "achieved": ach, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_F32_MFMA_TFLOPS,
                           "launches": n_l, "avg_launch_ms": ms / max(n_l, 1),
                           "executed_flops_per_launch": fl / max(n_l, 1),
                           "mfma_insts_per_launch": mfma_insts, "flop_per_mfma_inst": 2048,
                           "executed_flops_per_launch_from_counter": (mfma_insts * 2048.0) if mfma_insts else None,
                           # SURVEY 8(d)'s ALGORITHMIC count of the same launches; a fraction > 1 = multiply-adds avoided (Winograd 16 of 36, the
                           # unpooled source 9 of 36, zero sources skipped at step 0), never a faster pipe
                           "survey_8d_flops_per_launch": s8d_fl / max(n_l, 1),
                           "survey_8d_gmac_per_genome_step_by_layer": {str(l_): v / 1e9 for l_, v in s8d_layer.items()},
                           "survey_8d_tflops": s8d_fl / secs / 1e12,
                           "frac_on_survey_8d_flops": s8d_fl / secs / 1e12 / PEAK_F32_MFMA_TFLOPS,
                           "executed_over_survey_8d": fl / s8d_fl if s8d_fl else None,
                           "frac_note": "`frac` = executed multiply-adds / time / peak; `frac_on_survey_8d_flops` = SURVEY 8(d)'s 9-tap count of the same launches / the same time / peak",
                           "traffic": traffic, "traffic_commit": traffic_commit, "traffic_note": traffic_note,
                           "traffic_source": "profiles/pmc_summary_latest.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, bytes per launch)" if traffic else None,
                           # algorithmic HBM bytes of a launch: every source once + c in / out + h out (peepholes and weights are shared by the batch)
                           "traffic_algorithmic_bytes_by_layer": {str(l_): v for l_, v in alg_bytes.items()},
                           "traffic_algorithmic_bytes": alg_bytes_avg,
                           "traffic_over_algorithmic": (traffic / alg_bytes_avg) if traffic else None,
                           # whole path: the reference's formulation (9 taps on every source) vs what this build executes
                           "survey_8d_flops_per_genome": flops_step * N_STEPS_PREDNET,
                           "executed_flops_per_genome": all_fl / nb,
                           "whole_path_tflops_on_survey_8d_flops": flops_step * N_STEPS_PREDNET * out["value"] / 1e12,
                           "whole_path_frac_on_executed_flops": (all_fl / nb) * out["value"] / 1e12 / PEAK_F32_MFMA_TFLOPS,
                           "all_conv_kernels": allc,
                           "per_op": [{"layer": r["layer"], "op": r["epi"] + ("(step 0: zero sources skipped)" if r.get("step0") else ""), "ms": round(r["ms"], 3), "launches": r["launches"],
                                       "tflops": (r["flops_per_image"] * nb * r["launches"] / (r["ms"] * 1e-3) / 1e12) if r["ms"] > 0 else 0.0}
                                      for r in rows if r["launches"] > 0]}
        # The two HBM-side stages (SURVEY 8(d) "report both"): algorithmic bytes / HIP-event time of the stage / 8 TB/s -- and the
        # bound that actually binds them, which is not HBM: both move ~1 MB per genome.
        N = W * H
        n_in = 2
        render_bytes = nb * (C_DIM * N + n_in * N * 8)        # uint8 planes out + the float64 coordinate planes read per genome block
        flow_bytes = nb * int(2 * N * (1 + 0.25 + 1.0 / 16) * (1 + 2 * 2))  # 2 gray frames x 3 pyramid levels x (u8 + 2 x i16 derivatives)
        st = eng.timings()
        hb = []
        for name, b, msk, binds in (
                ("cppn_render_kernel (a2+a3)", render_bytes, "render_ms",
                 "fp64 VALU: ~25 nodes x (fdlibm exp / Cephes tanh, sin in float64, ~60-150 fp64 ops each) per pixel and genome; one pass over 1.25 MB per genome"),
                ("flow stage: gray, pyrDown, Scharr, min-eig, corner select, LK track (a6)", flow_bytes, "flow_ms",
                 "latency: one workgroup per image in corner_select_kernel (greedy min-distance selection is sequential in the corner rank) "
                 "and mineig_kernel; 10 dependent launches over 0.9 MB per genome")):
            t_ms = st[msk]
            a_ = b / (t_ms * 1e-3) / 1e12 if t_ms > 0 else 0.0
            hb.append({"bound": "hbm", "binding_bound": binds, "kernel": name, "algorithmic_bytes": b, "ms": t_ms, "achieved": a_, "peak": PEAK_HBM_TBS,
                       "unit": "TB/s", "frac": a_ / PEAK_HBM_TBS, "share_of_generation": t_ms / out["ms_per_step"]})
        out["roofline_hbm"] = hb
    grid = None
    if world == 1 and not args.no_cpu_baseline:
        grid = grids.create_grid(STRUCTURE, W, H, 10)
        cb, cpu_fit = cpu_baseline(cfg, population, wts, grid, shape, flops_per_genome=eng.flops_per_step() * N_STEPS_PREDNET, shape_name=args.shape)
        out["cpu_baseline"] = cb
        out["gpu_over_cpu"] = out["value"] / cb["value"]  # one CPU process at its best thread count
        if cb.get("whole_host", {}).get("value"):
            out["gpu_over_cpu_whole_host"] = out["value"] / cb["whole_host"]["value"]  # every CPU of the box busy
    if world == 1 and not args.no_parity:
        # (a) genome 0 at the FULL size against the bit-exact C oracle (~20 s of CPU): the canonical arithmetic, bit for bit
        import oracle as oracle_mod
        from oracle import pipeline
        grid = grid or grids.create_grid(STRUCTURE, W, H, 10)
        t1 = time.time()
        ref0 = pipeline.genome_fitness(genomes[0], cfg, grid, wts, CHANNELS, W, H, STRUCTURE)
        out["parity_check"] = {"genome": 0, "gpu": float(fit[0]), "oracle_c": float(ref0),
                               "rel_err": float(abs(fit[0] - ref0) / max(abs(ref0), 1e-300)) if ref0 != 0 else float(abs(fit[0])),
                               "oracle_seconds": time.time() - t1}
        # (b) EVERY genome of the population against the reference's element-wise order (north_star: 1e-4 relative)
        summ, fit2 = classify_population(eng, fitness, genomes, cfg, wts, shape)
        assert np.array_equal(fit2, fit[:len(fit2)]), "the staged entry points and the fused population path disagree"
        out["parity_check"]["population_vs_reference_order"] = summ
        out["parity_check"]["gate_order"] = {"hip": eng.lib.eigen_gate_order(), "oracle": oracle_mod.lib().eig_oracle_gate_order()}
        reasons = []
        if out["parity_check"]["rel_err"] > 1e-9:
            reasons.append("genome 0 differs from the bit-exact C oracle by %.3g" % out["parity_check"]["rel_err"])
        if summ["outside_1e-4_unexplained"]:
            reasons.append("%d genome(s) outside 1e-4 are not reproduced by +-1 byte flips of the HIP frames" % summ["outside_1e-4_unexplained"])
        if summ["max_byte_diff"] > 1 or summ["byte_flip_rate"] > 5e-5:
            reasons.append("frames differ from the reference-order frames by more than a sprinkling of +-1 bytes (max %d, rate %.2g)" % (summ["max_byte_diff"], summ["byte_flip_rate"]))
        if out["parity_check"]["gate_order"]["hip"] != out["parity_check"]["gate_order"]["oracle"]:
            reasons.append("HIP library and C oracle were compiled with different gate orders")
        out["parity_fail"] = bool(reasons)
        if reasons:
            out["parity_fail_reasons"] = reasons
            print("bench.py: PARITY FAILURE: " + "; ".join(reasons), file=sys.stderr)
    if world == 1 and not args.no_supplementary:
        # the other BASELINE.json configurations, same process, a few seconds each (driver-visible numbers)
        sup = {}
        fitness.clear_engines()
        torch.cuda.empty_cache()
        for name, pop_s, steps_s, key in (("ref160", 50, 20, "ref160 (the reference's own default shape, pop 50)"), ("c1", 10, 100, "configs[0] (on the GPU path)"), ("c2", 50, 60, "configs[1]"),   # (5-50 ms generations: 0.5-1 s each, or the box's host shows in the number)
                                          ("ref640", 16, 4, "ref640 (the reference's `--size big`, 640x480 colour, pop 16)"),
                                          ("c4", 512, 2, "configs[3] (single-GPU: two device batches of 256)"), ("c5", 64, 2, "configs[4] (single-GPU sample: one device batch of 64)"),
                                          # configs[4] at ITS population once -- 1024 genomes at 512x512 = four device batches of 256, one generation
                                          ("c5_full", 1024, 1, "configs[4] at its stated population (single GPU: four device batches of 256, ONE generation, warm-up = one more)")):
            try:
                r = supplementary_shape("c5" if name == "c5_full" else name, pop_s, steps_s, warmup=3 if steps_s >= 20 else 1, report_memory=(name == "c5_full"))
                r["config"] = key
                sup[name] = r
            except Exception as e:  # noqa: BLE001  (a supplementary failure must not cost the headline line)
                sup[name] = {"error": "%s: %s" % (type(e).__name__, e)}
            fitness.clear_engines()
            torch.cuda.empty_cache()
        out["supplementary"] = sup
    print(json.dumps(out))
    if args.strict_parity and out.get("parity_fail"):
        raise SystemExit(3)


if __name__ == "__main__":
    main()
