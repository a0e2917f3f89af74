"""GPU: a plain `bench.py --gpus 1 --steps N --warmup W` run and its `--dump-outputs DIR`.

* the plain line: N timed steps, `ms_per_step` and `value` of those steps, and none of the legs that
  run only under `--full`;
* the dumped arrays of a small C4 (every array below bench.DUMP_SAMPLE, so whole): the oracle's CSR
  and node names of the same generator bytes, element for element;
* bench.dump_array's sample of a larger array: the first and last run and the seeded runs between,
  the same elements on every call."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = 0.002  # C4 x 0.002: 100k S / 400k L
STEPS, WARMUP = 2, 1
FULL_ONLY = ("alt_paths", "other_configs", "scaling_reference", "cpu_baseline", "end_to_end")


@pytest.fixture(scope="module")
def plain_run(gpu, tmp_path_factory):
    out = tmp_path_factory.mktemp("dump")
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--scale", str(SCALE), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0]), out


def test_plain_line_is_the_timed_steps_alone(plain_run):
    line, _ = plain_run
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "M edge records/s" and line["higher_is_better"] is True
    assert line["metric"].startswith("M edges/sec GFA->CSR") and line["dtype"] == "u8/int64 (float64 weights)"
    assert line["ms_per_step"] > 0
    # value = edge records per second of the timed steps (both figures are rounded in the line)
    assert line["value"] == pytest.approx(line["config"]["n_links"] / (line["ms_per_step"] / 1e3) / 1e6, rel=2e-2)
    assert line["phase_ms"] and line["roofline"]["kernel"]
    assert not [k for k in FULL_ONLY if k in line]


def test_dumped_outputs_are_the_oracles_csr_and_names(plain_run, oracle_lib):
    from gfa2network_amd import synth

    line, out = plain_run
    wl = synth.WORKLOADS["C4"]
    n_s, n_l = int(wl.n_segments * SCALE), int(wl.n_links * SCALE)
    assert (line["config"]["n_segments"], line["config"]["n_links"]) == (n_s, n_l)
    o = oracle_lib.run(synth.host_bytes(n_s, n_l, seed=0, rc_tag=wl.rc_tag), **wl.mode)
    want = oracle_lib.to_raw(o, "csr")
    got = {p.stem: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["counts", "data", "indices", "indptr", "names_blob", "names_offsets"]
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["names_blob"].dtype == np.float32
    assert all(got[k].dtype == np.float64 for k in got if k != "names_blob")
    assert len(want.indices) <= bench.DUMP_SAMPLE  # whole arrays, not samples
    for k in ("indptr", "indices", "data", "names_offsets", "names_blob"):
        assert np.array_equal(got[k], getattr(want, k).astype(got[k].dtype)), k
    assert got["counts"].tolist() == [o.n_lines, o.n_records, n_l, o.n_nodes, len(want.indices),
                                      len(want.names_blob), 4]
    assert line["config"]["nnz"] == len(want.indices) and line["config"]["n_nodes"] == o.n_nodes


def test_dump_array_samples_a_large_array_at_fixed_runs(gpu, tmp_path):
    from gfa2network_amd import synth

    dev = synth.DeviceInput(30_000, 120_000)  # 2.9 MB of text: above DUMP_SAMPLE as bytes, below it as int32
    try:
        text = np.frombuffer(dev.download(), dtype=np.uint8)
        run, count = bench.DUMP_RUN, dev.len // 4
        assert dev.len > bench.DUMP_SAMPLE and count < bench.DUMP_SAMPLE
        bench.dump_array(str(tmp_path), "bytes", dev.ptr, dev.len, np.uint8, seed=7)
        bench.dump_array(str(tmp_path / "again"), "bytes", dev.ptr, dev.len, np.uint8, seed=7)
        bench.dump_array(str(tmp_path), "other_seed", dev.ptr, dev.len, np.uint8, seed=8)
        bench.dump_array(str(tmp_path), "words", dev.ptr, count, np.int32)
    finally:
        dev.free()
    got = np.load(tmp_path / "bytes.npy")
    assert got.dtype == np.float32 and len(got) == bench.DUMP_SAMPLE
    assert np.array_equal(got[:run], text[:run]) and np.array_equal(got[-run:], text[-run:])
    offs = np.sort(np.random.Generator(np.random.PCG64(7)).integers(0, dev.len - run, bench.DUMP_SAMPLE // run - 2))
    assert np.array_equal(got[run:-run], np.concatenate([text[o:o + run] for o in offs]))
    assert np.array_equal(got, np.load(tmp_path / "again" / "bytes.npy"))
    assert not np.array_equal(got, np.load(tmp_path / "other_seed.npy"))
    words = np.load(tmp_path / "words.npy")  # below DUMP_SAMPLE elements: the whole array, integers as float64
    assert words.dtype == np.float64 and np.array_equal(words, text[:count * 4].view(np.int32))
