"""GPU: bench.py at one rank.  A plain run times --steps steps and reports nothing that takes work of its own; --full adds the
digest, the probes and the PCIe-inclusive figure.  --dump-outputs writes the last timed step's outputs: the same from run to run
and with --full, and equal to the CPU oracle on the bench's own seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
import svtlibs
from svtlibs import ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096                                     # > DUMP_ROWS: the coefficient arrays are written as the seeded sample
NAMES = ("coeff", "qcoeff", "dqcoeff", "eob", "sad")


def run_bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "SVT_BENCH_SEED_RANK", "SVT_BENCH_PLACEMENT"):
        env.pop(k, None)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--blocks", str(N)] + list(extra), cwd=ROOT,
                        env=env, capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, (pr.stdout[-2000:], pr.stderr[-3000:])
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout[-2000:]
    return json.loads(lines[0])


def load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}


def test_plain_and_full_runs_and_dumped_outputs(tmp_path):
    a = run_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a"))
    b = run_bench("--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path / "b"))
    for r, steps in ((a, 3), (b, 5)):
        assert r["steps"] == steps and r["ms_per_step"] > 0 and r["value"] > 0 and r["unit"] == "blocks/s"
        assert r["higher_is_better"] is True and r["dtype"] == "i32" and r["roofline"]["frac"] > 0
        assert not {"cpu_baseline", "secondary", "digest_blocks_eob_sad_qchk"} & set(r)
        assert "box_fill_GBps" not in r["roofline"] and "contiguous_outputs_frac" not in r["roofline"]
    c = run_bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "c"))
    assert c["digest_blocks_eob_sad_qchk"][0] == N and "secondary" in c and "cpu_baseline" not in c
    assert c["roofline"]["box_fill_GBps"] > 0 and c["roofline"]["contiguous_outputs_frac"] > 0

    da, db, dc = load(tmp_path / "a"), load(tmp_path / "b"), load(tmp_path / "c")
    rows = bench.dump_index(N, bench.DUMP_ROWS)
    assert len(rows) == bench.DUMP_ROWS and bench.dump_index(N, bench.DUMP_SCALARS) is None
    assert sum(v.nbytes for v in da.values()) <= 64 * 10 ** 6
    for k in NAMES:
        assert da[k].dtype == np.float64 and da[k].shape == ((bench.DUMP_ROWS, 1024) if k.endswith("coeff") else (N,))
        assert np.array_equal(da[k], db[k]) and np.array_equal(da[k], dc[k]), k
    assert da["eob"].any() and da["sad"].all()

    # the bench's inputs (seed 13596, rank 0) through the CPU oracle, on a share of the dumped blocks
    g = torch.Generator(device="cuda:0"); g.manual_seed(13596)
    src = torch.randint(0, 256, (N, 32, 32), dtype=torch.uint8, device="cuda:0", generator=g).cpu().numpy()
    pred = torch.randint(0, 256, (N, 32, 32), dtype=torch.uint8, device="cuda:0", generator=g).cpu().numpy()
    qrow = {k: v[bench.QINDEX].copy() for k, v in svtlibs.quant_tables(8).items()}
    O = svtlibs.oracle()
    for j in range(0, bench.DUMP_ROWS, 8):
        i = int(rows[j])
        rc = np.zeros(1024, np.int32); rq = np.zeros(1024, np.int32); rdq = np.zeros(1024, np.int32)
        reob = np.zeros(1, np.uint16); rsad = np.zeros(1, np.uint32)
        O.svt_oracle_fwd_quant_sad(ptr(src[i]), 32, ptr(pred[i]), 32, 3, 0, ptr(qrow["zbin"]), ptr(qrow["round"]), ptr(qrow["quant"]),
                                   ptr(qrow["quant_shift"]), ptr(qrow["dequant"]), ptr(rc), ptr(rq), ptr(rdq), ptr(reob), ptr(rsad))
        assert np.array_equal(da["coeff"][j], rc) and np.array_equal(da["qcoeff"][j], rq) and np.array_equal(da["dqcoeff"][j], rdq), i
        assert da["eob"][i] == reob[0] and da["sad"][i] == rsad[0], i
