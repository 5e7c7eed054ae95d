"""bench.py's plain line and `--dump-outputs`: a plain run reports the headline only (everything else is `--full`), and the
dump holds what the last timed step handed back — the same bits as ops.pair_forward on the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("roofline", "single_call", "graph_cached", "checked_pairs", "check", "cpu_baseline")


def _outputs(P, N, seed):
    g = torch.Generator().manual_seed(seed)
    o = dict(warped=torch.rand(P, N, 3, generator=g), verts12=torch.rand(P, N, 3, generator=g),
             T12=torch.randint(0, N, (P, N), generator=g, dtype=torch.int32), losses=torch.rand(P, 6, generator=g))
    return o


def test_dump_outputs_names_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    import bench
    arrays = bench.host_outputs(_outputs(10, 64, 0), _outputs(10, 48, 1))
    assert sorted(arrays) == sorted("%s_%s" % (d, k) for d in ("out12", "out21") for k in ("warped", "verts12", "T12", "losses"))
    assert all(a.dtype == np.float32 and a.shape[0] == 10 for a in arrays.values())
    bench.dump_outputs(str(tmp_path / "all"), arrays)                       # under the budget: everything, no sample
    assert sorted(os.listdir(tmp_path / "all")) == sorted(k + ".npy" for k in arrays)
    assert np.array_equal(np.load(tmp_path / "all" / "out12_T12.npy"), arrays["out12_T12"])
    total = sum(a.nbytes for a in arrays.values())
    monkeypatch.setattr(bench, "DUMP_BYTES", total // 3)                     # over it: the same seeded pairs of every array
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == sorted(os.listdir(tmp_path / "s2")) and "sampled_pairs.npy" in files
    ids = np.load(tmp_path / "s1" / "sampled_pairs.npy")
    assert ids.dtype == np.float64 and 0 < len(ids) < 10 and np.all(np.diff(ids) > 0)
    assert sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in files) <= total // 3     # (128 = .npy header)
    for f in files:
        a, b = np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        if f != "sampled_pairs.npy":
            assert np.array_equal(a, arrays[f[:-4]][ids.astype(np.int64)])


def test_steps_must_be_positive():
    import bench
    assert bench.parse_args(["--steps", "3", "--warmup", "0"]).full is False
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


@pytest.mark.gpu
def test_plain_line_and_dump_match_the_pair_path(tmp_path):
    """A plain run: the headline fields, none of the --full ones.  Its dump = ops.pair_forward on the batch the last timed step
    consumed (steps + warmup = 4 pipeline steps over two alternating batches: the last one is batch 1, seed 5000), bit for bit."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--pairs", "8",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["full"] is False and not any(k in res for k in MOVED)
    assert res["unit"] == "pairs/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert abs(res["value"] - 8 * 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]

    sys.path.insert(0, os.path.join(ROOT, "dv-matcher_amd"))
    sys.path.insert(0, ROOT)
    import bench
    from dvm import ops
    dev = torch.device("cuda", 0)
    f1, f2, v1, v2, s1, s2 = bench.make_batch(8, 5000, dev)
    o12, o21 = ops.pair_forward(ops.deformer_weight_list(bench.load_weights(), dev), f1, f2, v1, v2, bench.ALPHA, s1, s2, with_map=True)
    want = bench.host_outputs(o12, o21)
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in want)
    for k, w in want.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float32 and got.shape == w.shape and np.array_equal(got, w), k
