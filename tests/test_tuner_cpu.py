"""hipps.ops.tuner without a GPU: recorded picks save / load (nested tuple keys, the committed
bench/tuner_picks.json), the candidate tables against the lists the dispatch sites have always
offered, and pick()'s cache rules."""
import importlib.util
import os
import subprocess
import sys

import pytest

from hipps.ops import tuner
from hipps.ops.tuner import _Tuner, g2_names, g2_parse, wgrad_names, wgrad_parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PICKS = os.path.join(ROOT, "bench", "tuner_picks.json")


def _bench():
    spec = importlib.util.spec_from_file_location("hipps_bench_main", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_save_load_round_trip(tmp_path):
    t = _Tuner()
    t.cache[("lfwd", 1024, 768, 768, True, False)] = "g2_256x256"  # flat
    t.cache[("1x1", 802816, 64, 64, 1, 56, 56, (True, False, False, False, False, False))] = "g2_128x64"  # epilogue
    t.cache[("wgrad", (256, 64, 56, 56), 256, 1, 1, 1, 0)] = "w3_0s3"  # shape tuple
    t.cache[("kxk", 256, 64, 56, 56, 64, 3, 1, 1, (True, None))] = "g2_128x64"  # None inside
    path = str(tmp_path / "picks.json")
    t.save(path)
    u = _Tuner()
    assert u.load(path) == 4
    assert u.cache == t.cache and list(u.cache) == list(t.cache)
    assert {hash(k) for k in u.cache} == {hash(k) for k in t.cache}


def test_load_reads_the_picks_file_as_bench_does():
    class Stub:
        def __init__(self):
            self.cache = {}

    s, u = Stub(), _Tuner()
    assert _bench()._load_picks(s, PICKS) == u.load(PICKS) == 76
    assert u.cache == s.cache and list(u.cache) == list(s.cache)


def _names_for(key):
    kind = key[0]
    if kind == "1x1":
        return ([] if key[7][5] else ["g1"]) + g2_names(key[3])
    if kind == "kxk":
        return ["miopen"] + g2_names(key[5])
    if kind == "pro":
        return g2_names(key[5], 2)
    if kind == "wgrad":
        return ["w2"] + wgrad_names(key[2], key[1][1], key[3] * key[4], "conv")
    if kind == "wgrad_pro":
        return wgrad_names(key[2], key[1][1], key[3] * key[4], "pro")
    assert kind == "bnpro", key
    return ["apply", "pro"]


def test_recorded_names_are_candidates():
    u = _Tuner()
    u.load(PICKS)
    assert {k[0] for k in u.cache} == {"1x1", "kxk", "pro", "wgrad", "wgrad_pro", "bnpro"}
    for key, name in u.cache.items():
        assert name in _names_for(key), (key, name)


def test_tuner_cache_env_loads_at_import():
    env = dict(os.environ, HIPPS_TUNER_CACHE=PICKS)
    out = subprocess.run([sys.executable, "-c", "import hipps.ops.nn as n; print(len(n.TUNER.cache))"], env=env,
                         cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == ["76"]


def test_g2_names_are_the_dispatch_sites_lists():
    assert g2_names(64) == ["g2_128x64", "g2_256x64", "g2_128x64s3"]
    assert g2_names(128) == ["g2_128x128", "g2_128x64", "g2_256x64", "g2_128x64s3"]
    assert g2_names(256) == ["g2_128x128", "g2_256x256", "g2_256x256s5", "g2_128x64", "g2_256x64", "g2_128x64s3"]
    # one stage count: the BN-prologue forward and the stride-2 input gradient offer 2-stage tiles
    assert g2_names(256, 2) == ["g2_128x128", "g2_256x256", "g2_128x64", "g2_256x64"]
    assert g2_names(64, 2) == ["g2_128x64", "g2_256x64"]
    assert g2_names(256, 5) == ["g2_256x256s5"]
    assert g2_parse("g2_256x256s5") == (256, 256, 5) and g2_parse("g2_128x64") == (128, 64, 2)
    for n in (64, 128, 256):
        for name in g2_names(n):
            bm, bn, ns = g2_parse(name)
            assert (bm, bn, ns) in tuner._G2_TILES and n % bn == 0


WGRAD = [
    ((256, 64, 1, "conv"), "w3_0 w3_0s3 w3_0s4"),
    ((64, 64, 9, "conv"), "w3_0 w3_0s3 w3_0s4 w3_5 w3_5s3 w3_6 w3_6s3"),
    ((512, 512, 9, "conv"), "w3_0 w3_0s3 w3_0s4 w3_1 w3_1s3 w3_2 w3_2s4 w3_3 w3_3s3 w3_4 w3_4s3"),
    ((768, 768, 1, "linear"), "w3_0 w3_0s3 w3_1 w3_1s3 w3_2 w3_2s4 w3_3 w3_3s3 w3_4 w3_4s3"),
    ((1024, 256, 1, "pro"), "w3_0 w3_1 w3_3 w3_4"),
    # (not in the issue's table: the remaining rules of each kind)
    ((64, 64, 9, "pro"), "w3_0 w3_5 w3_6"),  # multi-tap tiles on the prologue kernels, 2 stages only
    ((64, 64, 9, "linear"), "w3_0 w3_0s3"),  # a Linear has one tap: no cfg 5 / 6
    ((128, 256, 1, "conv"), "w3_0 w3_0s3 w3_0s4 w3_3 w3_3s3"),
    ((256, 128, 1, "conv"), "w3_0 w3_0s3 w3_0s4 w3_1 w3_1s3 w3_4 w3_4s3"),
]


@pytest.mark.parametrize("args,expect", WGRAD)
def test_wgrad_names_are_the_dispatch_sites_lists(args, expect):
    names = wgrad_names(*args)
    assert names == expect.split()
    for name in names:
        cfg, ns = wgrad_parse(name)
        assert name == f"w3_{cfg}" + ("" if ns == 2 else f"s{ns}")
        assert 0 <= cfg <= 6 and ns in (2, 3, 4)
    assert wgrad_parse("w3_2s4") == (2, 4) and wgrad_parse("w3_6") == (6, 2)


def test_pick_cache_rules():
    calls = []
    t = _Tuner()
    # one candidate: returned and stored without a measurement
    assert t.pick(("k", 1), ["only"], calls.append, calls.append) == "only"
    assert t.cache == {("k", 1): "only"} and not calls and not t.times
    # a cached name among the candidates: neither run nor timed is called
    t.cache[("k", 2)] = "b"
    assert t.pick(("k", 2), ["a", "b", "c"], calls.append, calls.append) == "b" and not calls
    # a recorded name that is no longer offered is a miss: the remaining candidate replaces it
    t.cache[("k", 3)] = "gone"
    assert t.pick(("k", 3), ["left"], calls.append) == "left"
    assert t.cache[("k", 3)] == "left" and not calls


def test_nn_exports_the_same_objects():
    from hipps.ops import nn as hnn

    assert hnn.TUNER is tuner.TUNER and hnn._Tuner is _Tuner
    assert hnn._g2_names is g2_names and hnn._g2_parse is g2_parse
    assert hnn.add_tune_quiet is tuner.add_tune_quiet and hnn.remove_tune_quiet is tuner.remove_tune_quiet
