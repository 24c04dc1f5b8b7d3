"""bench.py's plain run on the GPU: it times --steps steps, reports ms_per_step, runs none of the --full extras, and
--dump-outputs writes what its last timed step returns to a caller -- checked against the same evp(dt) calls made through
the Python binding, bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from cice5_amd import blocks, constants as C, dyn, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx,ny,xb,yb", [(240, 160, 4, 2), (720, 400, 6, 2)], ids=["whole_grid", "sampled"])
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path, nx, ny, xb, yb):
    ndte, dt, steps, warmup = 24, 1800.0, 3, 2
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--grid", f"{nx}x{ny}", "--xblocks", str(xb), "--yblocks", str(yb), "--ndte", str(ndte), "--dt", str(dt),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
    assert not {"verify", "cpu_baseline"} & set(line) and "open_variant" not in line["config"]

    # the same calls through the binding: state at rest, warm-up + timed steps of device-resident evp(dt)
    case = synth.SynthCase(nx=nx, ny=ny, ns_boundary=C.BND_NAMES["tripole"], land="continents", ice="polar", dt=dt, ndte=ndte)
    d = blocks.create_distrb_cart(nx, ny, nx // xb, ny // yb, ns_boundary_type="tripole")
    f = synth.make_block_fields(case, d)
    s = dyn.EvpDynamics(d, f, ndte=ndte, xmin=dyn.local_min_dx(f, d))
    s.init_evp(dt)
    s.ctx.upload(f)
    for _ in range(warmup + steps):
        s.ctx.prep(); s.ctx.subcycle(ndte); s.ctx.finish()
    names = synth.STATE_FIELDS + synth.OUTPUT_FIELDS + ["iceumask", "icetmask", "strength"]
    want = {n: np.zeros_like(f[n]) for n in names}
    s.ctx.download(want)
    s.close()

    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(tmp_path / (n + ".npy")) for n in names) <= 64 << 20
    cells = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(nx * ny, bench.DUMP_CELLS, replace=False)) \
        if nx * ny > bench.DUMP_CELLS else None
    for n in names:
        v = np.load(tmp_path / (n + ".npy"))
        g = blocks.gather_global(d, want[n]).astype(np.float64)
        assert v.dtype == np.float64
        assert np.array_equal(v, g if cells is None else g.ravel()[cells]), n
    assert np.load(tmp_path / "uvel.npy").any()
