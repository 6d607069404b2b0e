"""bench.py helpers that need no GPU: recorded kernel picks round-trip (nested tuple keys) and the
--dump-outputs writer (fixed seeded sample, float32, repeatable)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("hipps_bench_main", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Tuner:
    def __init__(self):
        self.cache = {}


def test_picks_round_trip_nested_keys(tmp_path):
    b = _bench()
    t = _Tuner()
    t.cache[("kxk", 256, 64, 56, 56, 64, 3, 1, 1, (True, None))] = "g2_128x64"
    t.cache[("wgrad", (256, 64, 56, 56), 64, 3, 3, 1, 1)] = "w3_0"
    t.cache[("bnpro", 256, 64, 56, 56, 256)] = "apply"
    path = str(tmp_path / "sub" / "picks.json")
    b._save_picks(t, path)
    u = _Tuner()
    u.cache[("bnpro", 256, 64, 56, 56, 256)] = "pro"  # a recorded key wins
    assert b._load_picks(u, path) == 3
    assert u.cache == t.cache
    assert all(isinstance(k, tuple) for k in u.cache)


def test_recorded_picks_file_loads_if_present():
    b = _bench()
    if os.path.exists(b.PICKS_FILE):
        u = _Tuner()
        assert b._load_picks(u, b.PICKS_FILE) == len(u.cache) > 0
        assert all(isinstance(k, tuple) and isinstance(v, str) for k, v in u.cache.items())


def test_dump_outputs_sample_is_fixed(tmp_path):
    b = _bench()
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(200, 200), torch.nn.Linear(200, 3))  # 40000 > DUMP_SAMPLE, rest whole
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    b._dump_outputs(d1, torch.tensor(2.5), m)
    b._dump_outputs(d2, torch.tensor(2.5), m)
    p1, p2 = np.load(os.path.join(d1, "params.npy")), np.load(os.path.join(d2, "params.npy"))
    assert p1.dtype == np.float32 and p1.shape == (b.DUMP_SAMPLE + 200 + 600 + 3,)
    assert np.array_equal(p1, p2)
    flat = torch.cat([p.detach().reshape(-1) for p in list(m.parameters())[1:]]).numpy()
    assert np.array_equal(p1[b.DUMP_SAMPLE:], flat)  # small parameters are written whole, in order
    w = m[0].weight.detach().reshape(-1).numpy()
    assert np.isin(p1[:b.DUMP_SAMPLE], w).all()
    loss = np.load(os.path.join(d1, "loss.npy"))
    assert loss.dtype == np.float32 and loss.tolist() == [2.5]
