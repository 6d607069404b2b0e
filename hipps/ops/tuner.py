"""Per-shape kernel choice by measurement, and the tables of GEMM candidates it chooses among (the
dispatch sites are in hipps.ops.nn).  Pure Python: importable without the native module."""
from __future__ import annotations

import contextlib
import json
import os

import torch

_TUNE_QUIET: list = []  # context-manager factories that keep other GPU work off while timing


def add_tune_quiet(fn) -> None:
    """Register ``fn() -> context manager`` to be entered around every tuner measurement (the
    co-located async PS registers a pause of its thread: its kernels would otherwise share the GPU
    with the timed candidates and skew the picks)."""
    _TUNE_QUIET.append(fn)


def remove_tune_quiet(fn) -> None:
    if fn in _TUNE_QUIET:
        _TUNE_QUIET.remove(fn)


def _tuples(v):
    return tuple(_tuples(i) for i in v) if isinstance(v, list) else v


class _Tuner:
    """Per-shape kernel choice by measurement (like cudnn.benchmark): on the first call for a
    key, every candidate runs once to warm up; then, with the device drained and the registered
    background work held (add_tune_quiet), ROUNDS rounds each time every candidate (2 calls between
    HIP events, candidates interleaved) and the fastest by its best round is cached.  Interleaved
    rounds and the minimum keep a transient neighbour (another stream's kernels) from deciding a
    pick: with the co-located PS running free a measured 35 % slower set of weight-gradient
    tilings was once picked (profiles/r5/emu/).  Candidates must be side-effect free apart from
    writing their output (every candidate writes the same values)."""

    ROUNDS = 3

    def __init__(self):
        self.cache: dict = {}  # key -> candidate name
        self.times: dict = {}  # key -> {name: ms}, for the keys measured in this process

    def pick(self, key, names, run, timed=None) -> str:
        """The name to launch for ``key`` among ``names`` (ordered; ties go to the earlier one).
        ``run(name)`` launches a candidate; ``timed(name)``, if given, is what gets measured
        instead (the candidate plus the work its choice leaves to the next kernel).  A recorded
        name that is no longer among ``names`` (picks older than the kernels) is measured again."""
        got = self.cache.get(key)
        if got is not None and got in names:
            return got
        if len(names) == 1:
            got = names[0]
        else:
            fn = timed or run
            for name in names:
                fn(name)
            with contextlib.ExitStack() as quiet:
                for q in list(_TUNE_QUIET):
                    try:
                        quiet.enter_context(q())
                    except Exception:  # (a quiet hook that cannot hold: measure anyway)
                        pass
                # drain every stream first: kernels still running on another stream (the weight-
                # gradient side stream, the PS stream) would otherwise share the GPU with the timing
                torch.cuda.synchronize()
                evs = {name: [] for name in names}
                for _ in range(self.ROUNDS):
                    for name in names:
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        fn(name)
                        fn(name)
                        e.record()
                        evs[name].append((s, e))
                torch.cuda.synchronize()
            t = self.times[key] = {name: min(s.elapsed_time(e) for s, e in pairs) / 2 for name, pairs in evs.items()}
            got = min(t, key=t.get)
        self.cache[key] = got
        return got

    def save(self, path: str) -> None:
        """Write every pick as JSON: a list of [key, candidate name]."""
        with open(path, "w") as f:
            json.dump([[k, v] for k, v in self.cache.items()], f)

    def load(self, path: str) -> int:
        """Adopt recorded picks (they win over measuring): runs that load the same file make the
        same choices, so choices between candidates that are not bitwise equal (weight-gradient
        slab counts, the BN prologue route) cannot differ between runs or ranks.  Keys come back
        as (nested) tuples.  Returns the number of picks read."""
        with open(path) as f:
            picks = json.load(f)
        for k, v in picks:
            self.cache[_tuples(k)] = v
        return len(picks)


TUNER = _Tuner()
# HIPPS_TUNER_CACHE=<file>: picks recorded by TUNER.save are loaded at import (set_deterministic)
if os.environ.get("HIPPS_TUNER_CACHE") and os.path.exists(os.environ["HIPPS_TUNER_CACHE"]):
    TUNER.load(os.environ["HIPPS_TUNER_CACHE"])

# gemm2.hip k_gemm tiles (block rows, block cols, LDS stages): 3 stages keep one tile's DMA in
# flight across every K-loop barrier (k_gemm NS).  Only 128x64 keeps two blocks per CU with 3
# stages; the others drop to one wave per SIMD and lose (profiles/gemm2_probe_r3_stages.json).
# (256, 256, 5): the ping-pong schedule of the 256x256 tile (k_gemm NS == 5)
_G2_TILES = ((128, 128, 2), (256, 256, 2), (256, 256, 5), (128, 64, 2), (256, 64, 2), (128, 64, 3))


def g2_names(N: int, stages=None):
    """The gemm2 tiles for N output columns, optionally only those with ``stages`` LDS stages."""
    return [f"g2_{bm}x{bn}" + ("" if ns == 2 else f"s{ns}") for bm, bn, ns in _G2_TILES
            if N % bn == 0 and stages in (None, ns)]


def g2_parse(name: str):
    """'g2_256x128s3' -> (256, 128, 3); 'g2_128x64' -> (128, 64, 2)"""
    t, _, ns = name[3:].partition("s")
    bm, bn = t.split("x")
    return int(bm), int(bn), int(ns or 2)


# gemm2.hip k_wgrad tilings (Cout x Cin*taps outputs), cfg -> (cout %, cin %): 0 128x128 (4 waves),
# 1 256x128 (4 waves), 2 256x256 (8 waves), 3 128x256 / 4 256x128 (8 waves of 64x64); 5 / 6: the
# 64-channel KxK layers only, two taps per 128-wide tile (K padded), 2 / 4 waves
_W3_DIV = {0: (1, 1), 1: (256, 128), 2: (256, 256), 3: (128, 256), 4: (256, 128), 5: (1, 1), 6: (1, 1)}
# kind -> {cfg: LDS stage counts offered}.  The three kinds differ on purpose:
#   conv:   every cfg; 3 stages do not fit 256x256 (cfg 2), which gets 4 (= 32-row k-half units, see
#           gemm2.hip) instead, as does cfg 0 on top of its 3
#   pro:    the BN-prologue kernels (nn._conv_wgrad_pro) run with 2 stages only and have no cfg 2
#   linear: a Linear's dW (one tap, so no cfg 5 / 6); as conv, but without the 4-stage cfg 0
# (fewer, longer M slabs -- gemm2_wgrad sdiv=2, half the fp32 slab traffic -- measured: no shape
# faster by more than 1 %, profiles/r3b/tuner_sdiv.json; not a candidate)
_W3_STAGES = {"conv": {0: (2, 3, 4), 1: (2, 3), 2: (2, 4), 3: (2, 3), 4: (2, 3), 5: (2, 3), 6: (2, 3)},
              "pro": {0: (2,), 1: (2,), 3: (2,), 4: (2,), 5: (2,), 6: (2,)},
              "linear": {0: (2, 3), 1: (2, 3), 2: (2, 4), 3: (2, 3), 4: (2, 3)}}


def wgrad_names(cout: int, cin: int, taps: int, kind: str):
    """The gemm2 weight-gradient candidates 'w3_<cfg>[s<stages>]' of a [cout, cin * taps] gradient;
    ``kind``: "conv", "pro" or "linear"."""
    names = []
    for cfg, stages in _W3_STAGES[kind].items():
        dn, dk = _W3_DIV[cfg]
        if cout % dn == 0 and cin % dk == 0 and (cfg < 5 or (cin == 64 and taps > 1)):
            names += [f"w3_{cfg}" + ("" if ns == 2 else f"s{ns}") for ns in stages]
    return names


def wgrad_parse(name: str):
    """'w3_2s4' -> (2, 4); 'w3_0' -> (0, 2): (cfg, LDS stages)"""
    cfg, _, ns = name[3:].partition("s")
    return int(cfg), int(ns or 2)
