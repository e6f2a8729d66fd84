#!/usr/bin/env python3
"""bench.py — headline metric of BASELINE.json:

    blocks/sec for the fused chain  residual -> FwdTxfm2d 32x32 DCT_DCT ->
    quantize_b_32x32 -> SAD 32x32, 8-bit, batched blocks resident in HBM.

A "step" is one pass of the hot path (one fused-kernel launch through the C ABI,
svt_hip_fwd_quant_sad_batch) over one batch of 2^20 synthetic blocks per GPU
(BASELINE.json configs[1]: "FwdTxfm2d + quantize 32x32 8-bit, 1M-block batch").
One process per GPU; blocks are sharded across ranks with no data-path
collective (weak scaling: per-GPU batch fixed); the only exchange is the
barrier + max-reduce of the elapsed time.

Prints ONE JSON line on rank 0, including
  roofline     algorithmic bytes (14 342 B/block) / average kernel
               duration measured with HIP events on the launch stream, vs the
               8 TB/s HBM3E peak (MI355X_MICROARCH.md)

A plain run only sets up, warms up, times --steps steps and prints the line.
--full adds what takes work of its own, after the timed steps:
  digest       [blocks, sum eob, sum sad, checksum(qcoeff)], all-reduced over ranks
  roofline.box_* / contiguous_outputs_* / clock figures  (skipped by --no-probes)
  secondary    the PCIe-inclusive figure (skipped by --no-probes)
  cpu_baseline the reference's own AVX2 kernels (oracle/_ref, built by
               oracle/Makefile from the reference sources) on the GPU box's
               host cores, bounded sample (skipped by --no-cpu-baseline)
--dump-outputs DIR writes the last timed step's outputs (rank 0) as .npy files.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BYTES_PER_BLOCK = 2 * 1024 + 3 * 4096 + 2 + 4      # 14 342
HBM_PEAK_GBS = 8000.0                               # MI355X HBM3E spec peak
QINDEX = 100
DUMP_SEED = 20260
DUMP_ROWS = 1 << 10             # coefficient rows --dump-outputs writes: 3 arrays x 1024 x 1024 float64 = 24 MiB
DUMP_SCALARS = 1 << 20          # eob / sad entries it writes: 2 x 2^20 float64 = 16 MiB


def host_cores():
    try:
        return len(os.sched_getaffinity(0))
    except AttributeError:
        return os.cpu_count() or 1


def host_cpu_info():
    """(model name, physical cores this process may run on) from /proc/cpuinfo; SMT siblings share a
    (physical id, core id) pair."""
    model, phys = "unknown", set()
    try:
        allowed = os.sched_getaffinity(0)
    except AttributeError:
        allowed = None
    try:
        cpu = pid = cid = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "processor":
                cpu, pid, cid = int(v), 0, None
            elif k == "model name":
                model = v
            elif k == "physical id":
                pid = int(v)
            elif k == "core id":
                cid = int(v)
            elif not k and cpu is not None:
                if allowed is None or cpu in allowed:
                    phys.add((pid, cid if cid is not None else cpu))
                cpu = None
    except OSError:
        pass
    return model, (len(phys) or host_cores())


def cpu_baseline_child(in_path, out_path, budget_s):
    """Runs in a CHILD process without torch / HIP (python bench.py --cpu-baseline-child ...): times the
    reference's production AVX2 path (kind 'reference', oracle/_ref) or, when that build is absent, the
    scalar oracle (kind 'port') over a bounded sample, and writes its outputs for the first blocks so
    that the parent can compare the GPU run bit for bit.  A crash here costs the bench its cpu_baseline
    object, never the GPU line."""
    import svtlibs
    P = svtlibs.ptr
    z = np.load(in_path)
    src_np, pred_np = z["src"], z["pred"]
    tabs = [np.ascontiguousarray(z[k]) for k in ("zbin", "round", "quant", "quant_shift", "dequant")]
    R = svtlibs.ref()
    logical = host_cores()
    model, physical = host_cpu_info()
    navail = src_np.shape[0]
    info = {"unit": "blocks/s", "cpu_model": model, "physical_cores": physical, "logical_cpus": logical}

    def run_ref(n, threads, keep, avx2=1):
        co = np.zeros((n, 1024), np.int32) if keep else None
        q = np.zeros((n, 1024), np.int32) if keep else None
        dq = np.zeros((n, 1024), np.int32) if keep else None
        eob = np.zeros(n, np.uint16); sad = np.zeros(n, np.uint32)
        t = R.ref_bench_fwd_quant_sad(P(src_np), P(pred_np), ctypes.c_size_t(n), threads, avx2, P(tabs[0]), P(tabs[1]),
                                      P(tabs[2]), P(tabs[3]), P(tabs[4]), P(co) if keep else None,
                                      P(q) if keep else None, P(dq) if keep else None, P(eob), P(sad))
        if t <= 0:
            raise RuntimeError("ref_bench_fwd_quant_sad reported a failed worker (see stderr)")
        return t, int(R.ref_bench_threads_used()), (co, q, dq, eob, sad)

    if R is not None:
        ncal = min(4096, navail)
        t1, _, _ = run_ref(ncal, 1, False)                    # calibrate, 1 thread
        rate1 = ncal / t1
        counts = sorted({physical, logical})                  # one thread per core, then SMT siblings too
        reps = 3                                              # best of 3 (a shared host is noisy; be fair to the CPU)
        per_rep = budget_s / (len(counts) * reps + 0.5)
        best = None
        for threads in counts:
            n = int(min(navail, max(ncal, rate1 * threads * per_rep * 0.6)))
            run_ref(min(n, 8192), threads, False)             # warm the pool / caches
            t, used = min(run_ref(n, threads, False)[:2] for _ in range(reps))
            leg = {"threads_asked": threads, "threads": used, "blocks": n, "value": n / t, "reps": reps}
            info.setdefault("legs", []).append(leg)
            if best is None or leg["value"] > best["value"]:
                best = leg
        # the scalar-C column of SURVEY 8(d) (residual_kernel_c, Av1TransformTwoD_32x32_c, aom_highbd_quantize_b_32x32_c,
        # fast_loop_nx_m_sad_kernel): one thread, then one thread per physical core
        nc1 = min(navail, 2048)
        tc1, _, _ = run_ref(nc1, 1, False, avx2=0)
        rate_c1 = nc1 / tc1
        ncp = int(min(navail, max(nc1, rate_c1 * physical * 0.7)))
        run_ref(min(ncp, 8 * physical), physical, False, avx2=0)      # start the pool once before timing it
        tcp, used_c = min(run_ref(ncp, physical, False, avx2=0)[:2] for _ in range(3))
        info.update({"value_scalar_c_1thread": rate_c1, "value_scalar_c": ncp / tcp, "scalar_c_threads": used_c,
                     "scalar_c_blocks": ncp})
        nv = min(navail, 16384)
        _, _, (co, q, dq, eob, sad) = run_ref(nv, min(logical, 64), True)
        info.update({"value": best["value"], "cores": best["threads"], "kind": "reference", "value_1thread": rate1,
                     "sample": f"{best['blocks']} of the step's blocks on {best['threads']} pthreads ({physical} physical "
                               f"cores / {logical} logical CPUs of {model}), reference AVX2 kernels (oracle/_ref), "
                               f"qindex {QINDEX}"})
    else:                                                    # no reference build here: scalar port
        O = svtlibs.oracle()
        n = nv = min(navail, 2048)
        co = np.zeros((n, 1024), np.int32); q = np.zeros((n, 1024), np.int32); dq = np.zeros((n, 1024), np.int32)
        eob = np.zeros(n, np.uint16); sad = np.zeros(n, np.uint32)
        t0 = time.perf_counter()
        for i in range(n):
            O.svt_oracle_fwd_quant_sad(P(src_np[i]), 32, P(pred_np[i]), 32, 3, 0, P(tabs[0]), P(tabs[1]), P(tabs[2]),
                                       P(tabs[3]), P(tabs[4]), P(co[i]), P(q[i]), P(dq[i]), P(eob[i:i + 1]),
                                       P(sad[i:i + 1]))
        info.update({"value": n / (time.perf_counter() - t0), "cores": 1, "kind": "port",
                     "sample": f"{n} blocks, 1 thread, scalar C oracle (oracle/_ref not present)"})
    np.savez(out_path, co=co[:nv], q=q[:nv], dq=dq[:nv], eob=eob[:nv], sad=sad[:nv], info=json.dumps(info))


def cpu_baseline(src_np, pred_np, qrow, gpu_out, budget_s=14.0):
    """cpu_baseline object of the JSON line: the child above, run as a separate process (the GPU process never
    loads oracle/ code), its stderr passed through, and the GPU outputs compared with its outputs."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory(prefix="svt_cpu_baseline_") as td:
        inp, outp = os.path.join(td, "in.npz"), os.path.join(td, "out.npz")
        np.savez(inp, src=src_np, pred=pred_np, **{k: np.ascontiguousarray(qrow[k]) for k in
                                                   ("zbin", "round", "quant", "quant_shift", "dequant")})
        env = dict(os.environ)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-child", inp, outp,
                             str(budget_s)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if pr.stderr:
            sys.stderr.write("[cpu_baseline stderr]\n" + pr.stderr[-4000:] + "\n")
        if pr.returncode != 0 or not os.path.exists(outp):
            return {"value": None, "unit": "blocks/s", "cores": 0, "kind": "reference",
                    "sample": "cpu baseline leg FAILED", "error": f"exit code {pr.returncode}",
                    "stderr_tail": pr.stderr[-600:]}
        z = np.load(outp)
        out = json.loads(str(z["info"]))
        nv = z["co"].shape[0]
        g_co, g_q, g_dq, g_eob, g_sad = gpu_out
        ok = (np.array_equal(g_co[:nv].cpu().numpy(), z["co"]) and np.array_equal(g_q[:nv].cpu().numpy(), z["q"])
              and np.array_equal(g_dq[:nv].cpu().numpy(), z["dq"])
              and np.array_equal(g_eob[:nv].cpu().numpy().view(np.uint16), z["eob"])
              and np.array_equal(g_sad[:nv].cpu().numpy().view(np.uint32), z["sad"]))
        out["gpu_equals_cpu_on_sample"] = bool(ok)
        out["verified_blocks"] = int(nv)
        return out


def dump_index(n, k):
    """the blocks --dump-outputs writes of an array of n blocks when at most k fit: None = all of them, else k sorted indices drawn
    from DUMP_SEED (the same for every run with the same --blocks)"""
    return None if n <= k else np.sort(np.random.default_rng(DUMP_SEED).choice(n, size=k, replace=False))


def dump_outputs(torch, outs, dirname):
    """--dump-outputs: what a caller of the timed path receives - coeff / qcoeff / dqcoeff [blocks, 1024], eob, sad [blocks] - as
    float64 .npy files (every value is an integer, exact in float64); at most DUMP_ROWS / DUMP_SCALARS blocks each (dump_index)."""
    os.makedirs(dirname, exist_ok=True)

    def sample(t, k):
        idx = dump_index(t.shape[0], k)
        return t if idx is None else t.index_select(0, torch.from_numpy(idx).to(t.device))
    co, q, dq, eob, sad = outs
    for name, t in (("coeff", co), ("qcoeff", q), ("dqcoeff", dq)):
        np.save(os.path.join(dirname, name + ".npy"), sample(t, DUMP_ROWS).cpu().numpy().astype(np.float64))
    np.save(os.path.join(dirname, "eob.npy"), sample(eob, DUMP_SCALARS).cpu().numpy().view(np.uint16).astype(np.float64))
    np.save(os.path.join(dirname, "sad.npy"), sample(sad, DUMP_SCALARS).cpu().numpy().view(np.uint32).astype(np.float64))


def box_probe(torch, dsp, dev, big, src, iters=5):
    """What THIS device delivers today, same process, outside the timed region (svt_hip_membw_probe: one 16-byte access per
    lane, grid as large as the job, non-temporal stores — the access shape of the fused kernel): a 4 GiB-class fill, a copy,
    and the kernel's own 1 : 6 read / write mix over the bench's own buffers.  GB/s of bytes moved (read + written)."""
    out = {}
    src_b = src.view(-1)
    nbytes_src = src_b.numel()
    third = big.numel() // 3
    a, b = big[:third], big[third:2 * third]

    def timed(fn, moved):
        fn(); fn()
        torch.cuda.synchronize()
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return moved / (e0.elapsed_time(e1) / iters * 1e-3) / 1e9

    out["box_fill_GBps"] = timed(lambda: dsp.membw_probe(0, big), big.numel() * 4)
    out["box_copy_GBps"] = timed(lambda: dsp.membw_probe(1, b, a), 2 * third * 4)
    if nbytes_src % 4096 == 0 and 6 * nbytes_src <= big.numel() * 4:
        out["box_mix_1r6w_GBps"] = timed(lambda: dsp.membw_probe(2, big, src_b), 7 * nbytes_src)
    return out


def clock_probe(torch, step, seconds=0.5):
    """The shader clock and board power the device HOLDS while the timed kernel runs: the hwmon files of the card whose PCI address is
    this device's, read from a thread while the kernel is replayed for ~ 0.5 s (outside the timed region).  Boxes whose memory probes
    read the same run the kernel 20 % apart; this is the other half of 'slow box or slow kernel'.  {} when the files are not there."""
    import glob
    import threading
    import time
    try:
        pr = torch.cuda.get_device_properties(torch.cuda.current_device())
        bdf = f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:{pr.pci_device_id:02x}.0"
        hw = glob.glob(f"/sys/bus/pci/devices/{bdf}/hwmon/hwmon*")
        if not hw:
            return {}
        hw = hw[0]

        def rd(name):
            try:
                return int(open(os.path.join(hw, name)).read().strip())
            except Exception:
                return None
        labels = {}
        for k in (1, 2):
            try:
                labels[open(os.path.join(hw, f"freq{k}_label")).read().strip()] = f"freq{k}_input"
            except Exception:
                pass
        f_s = labels.get("sclk", "freq1_input"); f_m = labels.get("mclk")
        stop, sclk, mclk, power, dpm = [False], [], [], [], {}

        def dpm_level(name):          # the level the driver marks current ('*') in pp_dpm_<name>, MHz
            try:
                for line in open(f"/sys/bus/pci/devices/{bdf}/pp_dpm_{name}").read().splitlines():
                    if line.rstrip().endswith("*"):
                        return int("".join(ch for ch in line.split(":")[1] if ch.isdigit()))
            except Exception:
                return None

        def sampler():
            while not stop[0]:
                v = rd(f_s)
                if v:
                    sclk.append(v / 1e6)
                if f_m:
                    v = rd(f_m)
                    if v:
                        mclk.append(v / 1e6)
                v = rd("power1_input")
                if v:
                    power.append(v / 1e6)
                if len(sclk) == 40:                      # once, in the middle of the loaded period: fabric / SoC / memory DPM levels
                    for nm in ("fclk", "socclk", "mclk"):
                        lv = dpm_level(nm)
                        if lv:
                            dpm[nm] = lv
                time.sleep(0.004)
        th = threading.Thread(target=sampler, daemon=True)
        t0 = time.perf_counter()
        for _ in range(4):
            step()
        torch.cuda.synchronize()
        th.start()
        while time.perf_counter() - t0 < seconds:
            for _ in range(8):
                step()
            torch.cuda.synchronize()
        stop[0] = True
        th.join(timeout=1.0)
        if not sclk:
            return {}
        med = lambda v: sorted(v)[len(v) // 2]
        out = {"sclk_MHz_under_load": round(med(sclk)), "sclk_MHz_min_max": [round(min(sclk)), round(max(sclk))], "clock_samples": len(sclk)}
        if mclk:
            out["mclk_MHz_under_load"] = round(med(mclk))
        if power:
            out["power_W_under_load"] = round(med(power))
        for nm, lv in dpm.items():
            out[f"{nm}_dpm_MHz_under_load"] = lv
        cap = rd("power1_cap")
        if cap:
            out["power_cap_W"] = round(cap / 1e6)
        return out
    except Exception as e:            # a diagnostic, never a reason to lose the line
        return {"clock_probe_error": str(e)[:120]}


def pcie_inclusive(torch, dsp, pkg, dev, src, pred, qrow, iscan, ns):
    """SURVEY 8(d) secondary figure: the same chain when the caller hands over HOST buffers — pinned host src / pred up,
    kernel, every output back down, one stream, no overlap between consecutive batches.  Never `value`."""
    hs, hp = src[:ns].cpu().pin_memory(), pred[:ns].cpu().pin_memory()
    ds, dp = torch.empty_like(src[:ns]), torch.empty_like(pred[:ns])
    douts = (torch.empty((ns, 1024), dtype=torch.int32, device=dev), torch.empty((ns, 1024), dtype=torch.int32, device=dev),
             torch.empty((ns, 1024), dtype=torch.int32, device=dev), torch.zeros(ns, dtype=torch.int16, device=dev),
             torch.zeros(ns, dtype=torch.int32, device=dev))
    houts = tuple(torch.empty(o.shape, dtype=o.dtype).pin_memory() for o in douts)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    best = None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        ds.copy_(hs, non_blocking=True); dp.copy_(hp, non_blocking=True)
        ev[1].record()
        dsp.fwd_quant_sad(ds, dp, pkg.TX_32X32, pkg.DCT_DCT, qrow, iscan, outs=douts)
        ev[2].record()
        for h, d in zip(houts, douts):
            h.copy_(d, non_blocking=True)
        ev[3].record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3]))
    dt, h2d_ms, k_ms, d2h_ms = best
    in_b, out_b = ns * 2048, ns * (3 * 4096 + 2 + 4)
    return {"metric": "blocks/s incl. PCIe (pinned host src+pred -> HBM, fused kernel, coeff+qcoeff+dqcoeff+eob+sad -> pinned host; "
                      "one stream, no overlap)", "value": ns / dt, "unit": "blocks/s", "sample_blocks": ns,
            "h2d_GBps": in_b / h2d_ms / 1e6, "d2h_GBps": out_b / d2h_ms / 1e6, "kernel_ms": k_ms,
            "note": "the boundary is device-resident (DESIGN 4.1); this is what a host-buffer caller would see"}


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--cpu-baseline-child":
        cpu_baseline_child(sys.argv[2], sys.argv[3], float(sys.argv[4]))
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=1 << 20, help="32x32 blocks per GPU per step")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also compute the output digest, the probes, the PCIe-inclusive figure and the CPU "
                         "baseline (a plain run only times the steps)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's outputs (rank 0) to DIR/<name>.npy, float64, a fixed sample of large arrays")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-probes", action="store_true",
                    help="with --full: skip the box fill / copy probe and the PCIe-inclusive secondary figure")
    ap.add_argument("--rehearse", action="store_true",
                    help="N > 1 on a ONE-GPU box: every rank uses cuda:0 and the process group is gloo (RCCL cannot put two ranks "
                         "on one device); walks exactly the multi-rank code path of the driver's 8-GPU run")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # One process per GPU.  Launched bare (`python bench.py --gpus N`, WORLD_SIZE unset) this process only starts the N
    # ranks as children and relays rank 0's line: it has imported neither torch nor the HIP library at this point.
    import __graft_entry__ as ge
    pkg = ge.load_package()
    from cidana_svt_av1_amd import launcher, sharding
    if launcher.needs_spawn(args.gpus):
        sys.exit(launcher.spawn_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    world = launcher.check_world(args.gpus)     # exits non-zero when WORLD_SIZE and --gpus disagree

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.rehearse else int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if args.rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    cdev = torch.device("cpu") if args.rehearse else dev      # where collective payloads live (gloo / RCCL)
    dsp = pkg.SvtHipDsp(local_rank)               # raises if the HIP library/device is unusable

    n = args.blocks
    g = torch.Generator(device=dev)
    g.manual_seed(13596 + int(os.environ.get("SVT_BENCH_SEED_RANK", rank)))   # seed constant of test/random.h:103; rank r draws stream 13596 + r (the variable lets a one-process run reproduce rank r's shard: tests)
    src = torch.randint(0, 256, (n, 32, 32), dtype=torch.uint8, device=dev, generator=g)
    pred = torch.randint(0, 256, (n, 32, 32), dtype=torch.uint8, device=dev, generator=g)
    qt = pkg.tables.quant_tables(8)               # the product's own host tables (oracle/ is used by the cpu_baseline leg only)
    qrow = {k: v[QINDEX].copy() for k, v in qt.items()}
    _, iscan_np = pkg.tables.scan_tables(pkg.TX_32X32, pkg.DCT_DCT)
    iscan = torch.from_numpy(iscan_np).to(dev)
    # Data layout in HBM: the three coefficient arrays the kernel writes at the same time are allocated FAR APART
    # (SvtHipDsp.alloc_spread = svt_hip_malloc_spread: 32 GiB spacers between them, freed again).  Inside one contiguous 12 GiB
    # allocation - how this bench placed them until round 3 - the same kernel runs 20 - 25 % slower on the same box, whatever the
    # skew between the arrays (profiles/r03_placement_probe*.log); a --full run still measures that placement below, outside the
    # timed region, and reports it as roofline.contiguous_outputs_*.  SVT_BENCH_PLACEMENT=contiguous times it as `value` instead.
    placement = os.environ.get("SVT_BENCH_PLACEMENT", "spread")
    # one 12 GiB allocation: the probes' buffer and the contiguous placement.  A plain run allocates it too (it is never touched), so that
    # the spread arrays below land where they land in a --full run.
    big = torch.empty(3 * n * 1024, dtype=torch.int32, device=dev)
    contiguous = (big[:n * 1024].view(n, 1024), big[n * 1024:2 * n * 1024].view(n, 1024), big[2 * n * 1024:].view(n, 1024))
    small = (torch.zeros(n, dtype=torch.int16, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    if placement == "spread":
        outs = tuple(dsp.alloc_spread([((n, 1024), torch.int32)] * 3)) + small
    else:
        outs = contiguous + small

    def step():
        dsp.fwd_quant_sad(src, pred, pkg.TX_32X32, pkg.DCT_DCT, qrow, iscan, outs=outs)

    for _ in range(args.warmup):
        step()

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    # HIP events on the stream the kernel is launched on (torch's current stream)
    stream = torch.cuda.current_stream(dev)
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record(stream)
    for _ in range(args.steps):
        step()
    ev1.record(stream)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kernel_ms = ev0.elapsed_time(ev1) / max(args.steps, 1)    # one kernel per step, back to back

    # ---- outside the timed region -----------------------------------------------------------------------------------
    if args.dump_outputs and rank == 0:
        dump_outputs(torch, outs, args.dump_outputs)
    digest = None
    if args.full:
        # digest of this rank's outputs: [blocks, sum eob, sum sad, checksum(qcoeff)] — ranks add (sharding.py)
        chk = 0
        for lo in range(0, n, 1 << 16):
            hi = min(n, lo + (1 << 16))
            w = (torch.arange(lo * 1024, hi * 1024, device=dev, dtype=torch.int64) % 8191) + 1
            chk = (chk + int(((outs[1][lo:hi].reshape(-1).to(torch.int64) * w) % sharding.DIGEST_MOD).sum().item())) % sharding.DIGEST_MOD
            del w
        digest = np.array([n, int((outs[3].to(torch.int64) & 0xffff).sum().item()),
                           int((outs[4].to(torch.int64) & 0xffffffff).sum().item()), chk], dtype=np.int64)
    per_rank = [kernel_ms]
    if world > 1:
        import torch.distributed as dist
        tt = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        km = [torch.zeros(1, dtype=torch.float64, device=cdev) for _ in range(world)]
        dist.all_gather(km, torch.tensor([kernel_ms], dtype=torch.float64, device=cdev))
        per_rank = [float(k.item()) for k in km]
        if args.full:
            digest = sharding.allreduce_digest(digest, None if args.rehearse else dev)

    result = None
    if rank == 0:
        total_blocks = n * world * args.steps
        achieved = BYTES_PER_BLOCK * n / (kernel_ms * 1e-3) / 1e9
        # HBM bytes per launch from the PMC counters are NOT measured by this run: they come from the committed profile of the
        # same command (tools/profile_round.sh: separate rocprofv3 --pmc passes); the line says which file, and for which
        # kernel build (git commit of the profiled tree) it stands.
        traffic = traffic_source = traffic_commit = None
        tpath = os.path.join(ROOT, "profiles", "traffic_latest.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("blocks") == n:
                    traffic = tj.get("hbm_bytes_per_launch")
                    traffic_source = tj.get("source")
                    traffic_commit = tj.get("commit")
            except Exception:
                traffic = None
        roofline = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                    "traffic_profiled_commit": traffic_commit,
                    "bytes_per_block": BYTES_PER_BLOCK, "kernel_ms": kernel_ms,
                    "kernel": "fwd32_kernel<IN_U8,QUANT,WITH_SAD>",
                    "per_rank": [{"rank": r, "kernel_ms": k, "achieved": BYTES_PER_BLOCK * n / (k * 1e-3) / 1e9,
                                  "frac": BYTES_PER_BLOCK * n / (k * 1e-3) / 1e9 / HBM_PEAK_GBS} for r, k in enumerate(per_rank)]}
        if args.full and not args.no_probes:
            # same process, same buffers, right after the timed steps: tells a slow box from a slow kernel
            roofline.update(box_probe(torch, dsp, dev, big, src))
            roofline["frac_of_box_fill"] = achieved / roofline["box_fill_GBps"]
            if "box_mix_1r6w_GBps" in roofline:
                roofline["frac_of_box_mix"] = achieved / roofline["box_mix_1r6w_GBps"]
            # the chain's own traffic and nothing else, on the SAME arrays: what this memory system gives the three-stream pattern here
            def chain():
                dsp.membw_probe_chain(src, pred, outs, n)
            for _ in range(2):
                chain()
            torch.cuda.synchronize()
            p0 = torch.cuda.Event(enable_timing=True); p1 = torch.cuda.Event(enable_timing=True)
            p0.record()
            for _ in range(5):
                chain()
            p1.record()
            torch.cuda.synchronize()
            pms = p0.elapsed_time(p1) / 5
            roofline["box_chain_traffic_only_ms"] = pms
            roofline["box_chain_traffic_only_GBps"] = 14336 * n / (pms * 1e-3) / 1e9
            roofline["kernel_over_traffic_only_time"] = kernel_ms / pms
            roofline.update(clock_probe(torch, step))      # (replays the timed kernel: the outputs are the step's again)
            if placement == "spread":
                # the same kernel with the three output arrays inside ONE 12 GiB allocation (the placement of rounds 1 - 3)
                couts = contiguous + small
                cstep = lambda: dsp.fwd_quant_sad(src, pred, pkg.TX_32X32, pkg.DCT_DCT, qrow, iscan, outs=couts)
                for _ in range(3):
                    cstep()
                torch.cuda.synchronize()
                c0 = torch.cuda.Event(enable_timing=True); c1 = torch.cuda.Event(enable_timing=True)
                c0.record()
                for _ in range(10):
                    cstep()
                c1.record()
                torch.cuda.synchronize()
                cms = c0.elapsed_time(c1) / 10
                roofline["contiguous_outputs_kernel_ms"] = cms
                roofline["contiguous_outputs_frac"] = BYTES_PER_BLOCK * n / (cms * 1e-3) / 1e9 / HBM_PEAK_GBS
            roofline["outputs_placement"] = "three arrays 32 GiB apart (svt_hip_malloc_spread)" if placement == "spread" else "one contiguous 12 GiB allocation"
            for _ in range(2):
                step()                          # the probes overwrote the outputs: restore them for the CPU comparison
            torch.cuda.synchronize()
        result = {
            "metric": "blocks/sec (FwdTxfm2d+quant+SAD, 32x32 8-bit)",
            "value": total_blocks / elapsed,
            "unit": "blocks/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            **({"rehearsal_all_ranks_on_one_gpu": True} if args.rehearse else {}),
            "vs_baseline": None,
            "dtype": "i32",
            "data": "synthetic",
            "config": {"workload": "configs[1]+SAD: fused residual->FwdTxfm2d 32x32 DCT_DCT->quantize_b_32x32->SAD, "
                                   "8-bit, qindex 100, uniform u8 src/pred",
                       "blocks_per_gpu": n, "global_blocks": n * world, "tx_size": "TX_32X32",
                       "tx_type": "DCT_DCT", "parallelism": f"block-range shard x{world}, no collective"},
            "roofline": roofline,
            **({"digest_blocks_eob_sad_qchk": [int(v) for v in digest]} if args.full else {}),
            "device": dsp.device_name(),
        }
        if args.full and world == 1 and not args.no_probes:
            result["secondary"] = pcie_inclusive(torch, dsp, pkg, dev, src, pred, qrow, iscan, min(n, 1 << 16))
        if args.full and world == 1 and not args.no_cpu_baseline:
            ns = min(n, 1 << 18)
            result["cpu_baseline"] = cpu_baseline(src[:ns].cpu().numpy(), pred[:ns].cpu().numpy(), qrow,
                                                  tuple(o[:ns] for o in outs))
            cb = result["cpu_baseline"]
            if cb.get("value"):
                result["gpu_over_cpu_avx2"] = result["value"] / cb["value"]
                result["target_10x_host_avx2_met"] = bool(result["value"] >= 10.0 * cb["value"])
        print(json.dumps(result), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
