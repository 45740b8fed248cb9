"""bench.py the way every change is measured: a plain run prints the headline line alone (what
--full adds is absent), and --dump-outputs writes what the last timed step returned.  Small size
(--versions 2: 8192 op files), one bench process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "kernels_ms_per_step", "variant_b", "strong", "host_buffers", "cpu_baseline",
             "configs")


def test_plain_run_headline_and_dump(tmp_path):
    import bench
    import crdtenc
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--versions", "2",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, timeout=200)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = p.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "op files/s" and line["dtype"] == "u32"
    assert line["higher_is_better"] is True and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["state_check"].endswith("ok")
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(4096 * 2 / (line["ms_per_step"] / 1e3), rel=1e-2)
    assert not [k for k in FULL_ONLY if k in line]
    # the dump: the last step's state file opens to the closed-form StateWrapper of this workload
    assert sorted(os.listdir(out)) == ["file_meta.npy", "state.npy"]
    st = np.load(out / "state.npy")
    meta = np.load(out / "file_meta.npy")
    assert st.dtype == np.float32 and meta.dtype == np.float32
    want = bench.expected_state(bench.actors_table(), 2)
    assert st.astype(np.uint8).tobytes() == want
    assert int(meta[0]) == 16 + crdtenc.sealed_len(len(want))
    assert meta[1:].astype(np.uint8).tobytes() == bench.APP
