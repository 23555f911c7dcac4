"""Group rounds (host_fit_schedule.hpp decides them, launch_fit_slots enqueues them; ANOFOX_HIP_TUNE group_launch): the specs of a class run each round in one launch of their class's
group kernel, on at most four streams.  Each problem's Nelder-Mead trajectory does not depend on which launch or lane runs it, so the
group schedule and the one-stream-per-spec schedule (group_launch=0) give the same bits, and so does every GPU_MAX_HW_QUEUES setting."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env(hiplib):
    import torch
    assert torch.cuda.is_available()
    from anofox_forecast_amd import synth
    return hiplib, synth


def _device_run(lib, Y, lens, model, h, tune, monkeypatch, **kw):
    import torch
    from anofox_forecast_amd.device import DeviceBatch
    monkeypatch.setenv("ANOFOX_HIP_TUNE", tune)
    n, T = Y.shape
    batch = DeviceBatch(n, T, lib.make_options(model, h, **kw), "cuda:0")
    block = torch.zeros((T, batch.ld), dtype=torch.float64, device="cuda:0")
    block[:, :n] = torch.from_numpy(np.ascontiguousarray(Y.T)).to("cuda:0")
    batch.set_block(block, torch.from_numpy(np.asarray(lens, dtype=np.int32)).to("cuda:0"))
    batch.run()
    torch.cuda.synchronize()
    r = batch.results()
    out = {k: r[k].cpu().numpy().copy() for k in ("yhat", "lower", "upper", "model_code", "status")}
    out["stats"] = batch.stats()
    return out


def _same(a, b, what):
    for k in ("yhat", "lower", "upper"):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert np.array_equal(a["model_code"], b["model_code"]), what
    assert np.array_equal(a["status"], b["status"]), what


def _ab(lib, Y, lens, monkeypatch, what, h=14, **kw):
    kw.setdefault("seasonal_period", 7)
    off = _device_run(lib, Y, lens, "AutoETS", h, "group_launch=0", monkeypatch, **kw)
    on = _device_run(lib, Y, lens, "AutoETS", h, "group_launch=1", monkeypatch, **kw)
    one = _device_run(lib, Y, lens, "AutoETS", h, "group_launch=1;group_split=0", monkeypatch, **kw)
    _same(off, on, what)
    _same(off, one, what + " (one general group)")
    return on


def test_positive_m5_subsample(env, monkeypatch):
    lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 0, 4000, 400, 7, positive=True)
    lens = [400 - (s % 7) * 11 for s in range(4000)]
    _ab(lib, Y, lens, monkeypatch, "positive M5 sub-sample")


def test_raw_intermittent_counts(env, monkeypatch):
    lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 0, 3000, 300, 7, positive=False)
    _ab(lib, Y, [300] * 3000, monkeypatch, "raw intermittent counts")


def test_two_shard_run(env, monkeypatch):
    """A shard of a 2-GPU job on the M5 shape (15,245 series): the first round deals four lanes per problem by expected work."""
    lib, synth = env
    from anofox_forecast_amd import dist
    n = 30490
    for r in range(2):
        a, b = dist.shard_range(n, r, 2)
        Y = synth.gen_series(synth.SEED_M5, a, b - a, 240, 7, positive=True)
        _ab(lib, Y, [240] * (b - a), monkeypatch, f"shard {r} of 2", h=28)


def test_tiny_batch(env, monkeypatch):
    lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 77, 12, 90, 7, positive=True)
    _ab(lib, Y, [90 - s for s in range(12)], monkeypatch, "tiny batch")


def test_fixed_period_24(env, monkeypatch):
    lib, synth = env
    Y = synth.gen_series(synth.SEED_M5, 300, 700, 24 * 12, 24, positive=True)
    _ab(lib, Y, [24 * 12 - (s % 3) * 24 for s in range(700)], monkeypatch, "m = 24", h=24, seasonal_period=24)


_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %r)
    import numpy as np
    from anofox_forecast_amd import api, lib, synth
    Y = synth.gen_series(synth.SEED_M5, 11, 2500, 260, 7, positive=True)
    got, berr = api.forecast_batch(list(Y), lib.make_options("AutoETS", 14, seasonal_period=7))
    assert berr["ok"], berr
    np.save(sys.argv[1], np.array([np.asarray(g["point"], dtype=np.float64) for g in got]))
    print("OK")
""") % ROOT


def test_hardware_queue_settings_give_identical_outputs(tmp_path):
    """Fresh processes with GPU_MAX_HW_QUEUES unset, 4 and 16 (the fit schedule does not depend on it): the same forecasts."""
    outs = []
    for q in (None, "4", "16"):
        envv = dict(os.environ)
        envv.pop("GPU_MAX_HW_QUEUES", None)
        if q is not None:
            envv["GPU_MAX_HW_QUEUES"] = q
        path = str(tmp_path / f"q{q}.npy")
        out = subprocess.run([sys.executable, "-c", _CHILD, path], env=envv, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stderr[-2000:]
        outs.append(np.load(path))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
