"""The measuring protocol of the tools/*_timing.py scripts, stated once.  A timing tool describes WHAT it measures -- its scene, its byte model,
a dict of calls, the ratios it derives and the wording of its record -- and takes everything else from here:

  * a Clock times one call in milliseconds: a pair of device events around it (on the stream given, else on torch's current stream) and then a
    synchronise (torch.cuda.synchronize unless the tool names another, e.g. its context's).  device="cpu" is the host clock around
    `f(); sync()`: the simulator rehearsals (--lib PATH --device cpu), and the whole calls that end on the host or synchronise themselves, which
    the speckle, confidence, eval and reproject tools have always taken with the host clock on the GPU too;
  * time_calls warms every call of a group `warm` times, synchronises once, and then takes `timings` rounds; a round times every call once, in
    the dict's order, so a drift of the machine hits the calls of a group alike.  A call measured on its own is a group of one (time_one).
    `burst` adds `burst_rounds` rounds that time `burst` back-to-back launches of each call between one pair of events and report the time per
    launch, which leaves the launch gap out;
  * spread is the one summary of a sample: median, min, max, n.  The figure a tool quotes is the median;
  * copy_call is the yardstick: les_hip_calib_copy (dword per lane) or _wide (16 bytes per lane) over as many floats as move the kernel's
    bytes -- a copy of n floats reads 4 n and writes 4 n bytes, so n = ceil(bytes / 8), for the wide copy rounded up to a multiple of 4 --
    of random floats;
  * write_record prints the record and writes it.
Nothing measured here is a gate."""
import ctypes as C
import json
import os
import time

import numpy as np


def spread(values, digits=None, samples=False):
    """median, min, max and n of a sample, rounded to `digits` places (None: as measured); samples=True adds the values, to 4 places."""
    v = np.asarray(values, np.float64)
    if v.size == 0:
        raise ValueError("spread: an empty sample")
    r = (lambda x: float(x)) if digits is None else (lambda x: round(float(x), digits))
    out = dict(median=r(np.median(v)), min=r(v.min()), max=r(v.max()), n=int(v.size))
    if samples:
        out["samples"] = [round(float(x), 4) for x in v]
    return out


class Clock:
    """time(f) -> milliseconds of one call of f (see the module's docstring).  sync() is the synchronise it ends every timing with."""

    def __init__(self, torch, device, stream=None, sync=None):
        self.torch, self.gpu, self.stream = torch, device != "cpu", stream
        self.sync = sync or (torch.cuda.synchronize if self.gpu else (lambda: None))

    def time(self, f):
        if not self.gpu:
            t0 = time.perf_counter()
            f()
            self.sync()
            return (time.perf_counter() - t0) * 1e3
        ev0, ev1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        ev0.record(self.stream)
        f()
        ev1.record(self.stream)
        self.sync()
        return ev0.elapsed_time(ev1)


def time_calls(clock, calls, timings, warm, burst=0, burst_rounds=5):
    """({name: [ms of one call, ...]}, {name: [ms per launch of a burst, ...]}) of the ordered {name: callable} `calls`."""
    for f in calls.values():
        for _ in range(warm):
            f()
    sync = getattr(clock, "sync", None)
    if sync:
        sync()
    single, bursts = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(timings):
        for k, f in calls.items():
            single[k].append(clock.time(f))

    def launches(f):
        for _ in range(burst):
            f()
    for _ in range(burst_rounds if burst > 0 else 0):
        for k, f in calls.items():
            bursts[k].append(clock.time(lambda: launches(f)) / burst)
    return single, bursts


def time_one(clock, f, timings, warm):
    """[ms, ...] of a call measured on its own: a group of one."""
    return time_calls(clock, {"call": f}, timings, warm)[0]["call"]


def copy_floats(nbytes, wide=False):
    """The floats a copy reads AND writes to move `nbytes` in total (8 bytes per float); the wide copy takes a multiple of 4."""
    n = (int(nbytes) + 7) // 8
    return (n + 3) // 4 * 4 if wide else n


def copy_call(api, nbytes, stream, wide=False, device=0, lib=None, random=True):
    """A callable that launches les_hip_calib_copy (wide: _wide) over copy_floats(nbytes, wide) floats of buffers of its own on `stream` (an
    address or None); .floats is that count, .buffers the source and the destination.  The source holds random floats; random=False makes it
    zeros, which is what the planefit, reproject and speckle records were taken with (their sources were fresh, never written allocations; the
    MI355X copies zeros up to 13 % faster than random floats when the buffers fit the last-level cache).  device="cpu" puts the buffers on the host, for a rehearsal
    on the simulator build `lib`."""
    import torch
    n = copy_floats(nbytes, wide)
    where = "cpu" if device == "cpu" else f"cuda:{device}"
    src, dst = (torch.rand if random else torch.zeros)(n, device=where), torch.empty(n, device=where)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0             # (the wide copy moves 16 bytes per lane)
    L = api.load(lib)
    entry = L.les_hip_calib_copy_wide if wide else L.les_hip_calib_copy
    args = (C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), C.c_size_t(n), 0 if device == "cpu" else device, C.c_void_p(stream or None))

    def call():
        api._chk_lib(L, entry(*args))
    call.floats, call.buffers = n, (src, dst)
    return call


def require_gpu(tool_name):
    """torch, or the error of a measuring tool that finds no HIP device (there is no fall-back to the host clock)."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool_name} measures on the GPU: no HIP device")
    return torch


def device_label(torch):
    return f"{torch.cuda.get_device_name(0)} ({getattr(torch.cuda.get_device_properties(0), 'gcnArchName', '?')})"


def write_json(path, rec):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)


def write_text(path, text):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def write_record(out, rec, md=None):
    """Prints the record as JSON; with `out` (a path with or without its .json) writes <out>.json and, when `md` (text) is given, <out>.md."""
    print(json.dumps(rec, indent=1), flush=True)
    if out:
        stem = out[:-len(".json")] if out.endswith(".json") else out
        write_json(stem + ".json", rec)
        if md is not None:
            write_text(stem + ".md", md)
