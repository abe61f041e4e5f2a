"""The measuring protocol of the timing tools (tools/timing.py) on the CPU: the spread, the order of a group's calls, the host clock, the sizing of
the own-copy reference, the record on disk -- and that every tools/*_timing.py takes them from there.  No library build, no device."""
import glob
import importlib.util
import inspect
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
CONVERTED = sorted(glob.glob(os.path.join(TOOLS, "*_timing.py")))
QUEUE_ALL = ("bf_timing.py", "interp_timing.py", "vdisp_timing.py")     # queue every pair of events, synchronise once: their loop stayed


def _load(path, monkeypatch):
    """The module at `path`, imported as the tools import each other (tools/ on sys.path), leaving sys.path, sys.modules and the environment alone."""
    monkeypatch.setattr(sys, "path", [TOOLS] + sys.path)
    monkeypatch.setattr(os, "environ", os.environ.copy())
    before = set(sys.modules)
    try:
        spec = importlib.util.spec_from_file_location("_tool_under_test_" + os.path.basename(path)[:-3], path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        for name in set(sys.modules) - before:
            if getattr(sys.modules[name], "__file__", None) and os.path.dirname(sys.modules[name].__file__) == TOOLS:
                del sys.modules[name]


@pytest.fixture()
def timing(monkeypatch):
    return _load(os.path.join(TOOLS, "timing.py"), monkeypatch)


def test_spread(timing):
    assert timing.spread([3, 1, 2]) == dict(median=2.0, min=1.0, max=3.0, n=3)
    v = [1.23456, 2.34567, 9.87654]
    assert timing.spread(v, digits=3) == dict(median=2.346, min=1.235, max=9.877, n=3)
    assert timing.spread(v, digits=None) == dict(median=2.34567, min=1.23456, max=9.87654, n=3)
    assert timing.spread(v, samples=True)["samples"] == [1.2346, 2.3457, 9.8765] and "samples" not in timing.spread(v)
    with pytest.raises(ValueError):
        timing.spread([])


class FakeClock:
    def __init__(self):
        self.n, self.syncs_at = 0, []

    def bind(self, log):
        self.log = log
        return self

    def time(self, f):
        f()
        self.n += 1
        return float(self.n)

    def sync(self):
        self.syncs_at.append(len(self.log))


def test_time_calls_order(timing):
    log = []
    calls = {k: (lambda k=k: log.append(k)) for k in ("b", "a", "c")}
    clock = FakeClock().bind(log)
    single, burst = timing.time_calls(clock, calls, timings=4, warm=2)
    assert log == ["b", "b", "a", "a", "c", "c"] + ["b", "a", "c"] * 4
    assert clock.syncs_at == [6]                                  # one synchronise, after the warm-up
    assert list(single) == ["b", "a", "c"] and all(len(v) == 4 for v in single.values())
    assert single["b"] == [1.0, 4.0, 7.0, 10.0] and single["c"] == [3.0, 6.0, 9.0, 12.0]
    assert burst == dict(b=[], a=[], c=[])
    assert timing.time_one(FakeClock().bind([]), lambda: None, 3, 0) == [1.0, 2.0, 3.0]


def test_time_calls_burst(timing):
    log = []
    calls = {k: (lambda k=k: log.append(k)) for k in ("x", "y")}
    clock = FakeClock().bind(log)
    single, burst = timing.time_calls(clock, calls, timings=1, warm=0, burst=5, burst_rounds=2)
    assert log == ["x", "y"] + (["x"] * 5 + ["y"] * 5) * 2
    assert single == dict(x=[1.0], y=[2.0])
    assert burst == dict(x=[3.0 / 5, 5.0 / 5], y=[4.0 / 5, 6.0 / 5])     # one reading per five launches, reported per launch


def test_time_calls_clock_without_sync(timing):
    class Bare:
        def time(self, f):
            f()
            return 1.0
    assert timing.time_calls(Bare(), dict(f=lambda: None), 2, 1)[0] == dict(f=[1.0, 1.0])


def test_clock_host_mode(timing):
    n = dict(f=0, sync=0)
    clock = timing.Clock(None, "cpu", sync=lambda: n.__setitem__("sync", n["sync"] + 1))
    ms = clock.time(lambda: n.__setitem__("f", n["f"] + 1))
    assert n == dict(f=1, sync=1) and ms >= 0.0


def test_copy_floats(timing):
    nbytes = 15 * 992 * 1436
    assert timing.copy_floats(nbytes) == (nbytes + 7) // 8 == 2670960
    assert timing.copy_floats(8 * 1000) == 1000 and timing.copy_floats(8 * 1000 + 1) == 1001
    for nb in (nbytes, 29 * 992 * 1436, 8 * 1001, 1):
        n = timing.copy_floats(nb, wide=True)
        assert n % 4 == 0 and 0 <= n - timing.copy_floats(nb) < 4


class StubLib:
    def __init__(self):
        self.calls = []

    def les_hip_calib_copy(self, *a):
        self.calls.append(("copy",) + a)
        return 0

    def les_hip_calib_copy_wide(self, *a):
        self.calls.append(("wide",) + a)
        return 0


class StubApi:
    def __init__(self):
        self.L, self.loaded, self.checked = StubLib(), [], []

    def load(self, path=None):
        self.loaded.append(path)
        return self.L

    def _chk_lib(self, L, rc):
        self.checked.append(rc)


@pytest.mark.parametrize("wide", [False, True])
def test_copy_call(timing, wide):
    api, nbytes = StubApi(), 15 * 992 * 1436 + (4 if wide else 0)
    call = timing.copy_call(api, nbytes, None, wide=wide, device="cpu", lib="sim.so")          # (host buffers: the rehearsal's mode)
    assert call.floats == timing.copy_floats(nbytes, wide) and (not wide or call.floats % 4 == 0)
    assert api.loaded == ["sim.so"] and api.L.calls == []
    call()
    call()
    assert api.checked == [0, 0] and len(api.L.calls) == 2
    name, src, dst, n, device, stream = api.L.calls[0]
    assert name == ("wide" if wide else "copy") and n.value == call.floats and device == 0 and stream.value is None
    assert (src.value, dst.value) == tuple(b.data_ptr() for b in call.buffers) and src.value % 16 == 0 and dst.value % 16 == 0
    assert all(b.numel() == call.floats for b in call.buffers)
    zeros = timing.copy_call(api, 64, None, device="cpu", random=False)
    assert zeros.floats == 8 and not zeros.buffers[0].any() and call.buffers[0].any()


def test_write_record(timing, tmp_path, capsys):
    rec = dict(shape=[3, 2], us=dict(a=dict(median=1.5, n=2)), text="x")
    timing.write_record(None, rec, "unused")
    assert json.loads(capsys.readouterr().out) == rec and os.listdir(tmp_path) == []
    out = tmp_path / "deep" / "er" / "rectify"                    # neither directory exists
    timing.write_record(str(out), rec, "# title\n")
    assert json.load(open(str(out) + ".json")) == rec and open(str(out) + ".md").read() == "# title\n"
    timing.write_record(str(tmp_path / "plain.json"), rec)        # a tool whose --out names the .json itself
    assert json.load(open(tmp_path / "plain.json")) == rec and sorted(os.listdir(tmp_path)) == ["deep", "plain.json"]


def test_nineteen_tools():
    assert len(CONVERTED) == 19 and all(q in map(os.path.basename, CONVERTED) for q in QUEUE_ALL)


@pytest.mark.parametrize("path", CONVERTED, ids=[os.path.basename(p) for p in CONVERTED])
def test_tool_states_no_protocol_of_its_own(path, monkeypatch):
    mod = _load(path, monkeypatch)
    own = {name for name, f in inspect.getmembers(mod, inspect.isfunction) if f.__module__ == mod.__name__}
    assert not own & {"_spread", "_med", "_timed", "_events", "_host_timed"}
    assert "Clock" not in {name for name, c in inspect.getmembers(mod, inspect.isclass) if c.__module__ == mod.__name__}
    text = open(path).read()
    assert ("cuda.Event(" in text) == (os.path.basename(path) in QUEUE_ALL)
    assert "tools/timing.py" in mod.__doc__ or os.path.basename(path) in QUEUE_ALL
    imported = {os.path.basename(getattr(v, "__file__", None) or "") for v in vars(mod).values() if inspect.ismodule(v)}
    assert "timing.py" in imported


def test_harness_holds_the_events():
    assert "cuda.Event(" in open(os.path.join(TOOLS, "timing.py")).read()
