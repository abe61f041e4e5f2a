"""Every compiled unary-cost kernel instantiation (csrc/les_hip_march_tables.inc) at its radius, route and job cut, shared by the simulator
tests (-m "not gpu") and the MI355X tests (-m gpu) of tests/test_instantiations.py.

The census parses the tables and requires that the matrix below names exactly the compiled set, so an instantiation added without a test
fails the suite.  The references are the existing ones: the oracle (volume energy at interpolation 1, image-based energy at v = 0),
InterpPair.expected (interpolation 0 / 2), bilateral_cases.bf_ref (through BfPair) and the vdisp_cases restatement (v != 0).  Every
comparison counts the finite, non-sentinel pixels it compared and fails below a floor, so that an all-NaN or all-sentinel output cannot pass.

March cuts: LES_HIP_MARCH_WIDE picks the entry (1: WGC 256, one job per workgroup; 0: WGC 128, two jobs), LES_HIP_MARCH_ROWS the rows per
job; both are read when a batch is created.  Every cut of one batch must give the same bits, and les_hip_batch_num_jobs must equal the
workgroup count of the forced cut (tw / TW balanced strips, th / rows balanced chunks, padded to NJ)."""
import contextlib
import os
import re

import numpy as np

from localexpstereo_amd import api, synth
from oracle import oracle as om
from tests import bilateral_cases as bc
from tests import interp_cases as ic
from tests import parity_cases as pc
from tests import vdisp_cases as vc

TABLES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "localexpstereo_amd", "csrc", "les_hip_march_tables.inc")
SENT = np.float32(1e6)
F32 = np.float32

# ------------------------------------------------------------------------------------------------ the matrix the tests run
MARCH_BY = {2: 2, 3: 3, 4: 3, 5: 4, 6: 5, 7: 5, 8: 6, 9: 7, 10: 7}          # radius -> rows per block (both entries)
MARCH_ENTRIES = {"wide": (256, 1), "narrow": (128, 2)}                      # entry -> (columns per job slot WGC, job slots per workgroup NJ)
STRIP_RADII = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 15)
STRIP_VARIANTS = {10: (8, 11)}                                              # LES_HIP_VARIANT entries besides variant 0
STRIP_FAMILIES = ("strip", "naive", "nearest", "quadratic")
ROW_OPTS = (1 << 30, 1024, 512, 384, 256, 192, 128, 96, 64, 48, 32)        # build_march_jobs' candidate rows per job


def matrix():
    """(family, radius, entry) of every instantiation the tests of test_instantiations.py run."""
    s = set()
    for R, BY in MARCH_BY.items():
        for wgc, nj in MARCH_ENTRIES.values():
            s.add(("march", R, (wgc, nj, BY)))
    for fam in STRIP_FAMILIES:
        for R in STRIP_RADII:
            s.add((fam, R, 0))
    for R, vs in STRIP_VARIANTS.items():
        for v in vs:
            s.add(("strip", R, v))
    return s


def census(text=None):
    """(family, radius, entry) of every instantiation in les_hip_march_tables.inc as the product compiles it (no macro defined: blocks
    under LES_MARCH_LAB drop out, their #else branches stay)."""
    text = open(TABLES).read() if text is None else text
    text = re.sub(r"//[^\n]*", "", text)
    lines, stack = [], []
    for ln in text.replace("\\\n", " ").split("\n"):
        s = ln.strip()
        if s.startswith("#if"):
            cond = s[3:].strip()
            if s.startswith("#ifdef"):
                cond = "defined(%s)" % s[6:].strip()
            elif s.startswith("#ifndef"):
                cond = "!defined(%s)" % s[7:].strip()
            expr = re.sub(r"defined\s*\(?\s*\w+\s*\)?", "False", cond).replace("&&", " and ").replace("||", " or ")
            expr = re.sub(r"!(?!=)", " not ", expr)
            stack.append([bool(eval(expr)), all(a for a, _ in stack)])
        elif s.startswith("#else"):
            stack[-1][0] = not stack[-1][0]
        elif s.startswith("#endif"):
            stack.pop()
        elif all(a for a, _ in stack):
            lines.append(ln)
    text = "\n".join(lines)

    def body(name):
        m = re.search(r"\b%s\s*\[\s*\]\s*=\s*\{(.*?)\};" % name, text, re.S)
        assert m, f"{name} not found in {TABLES}"
        return m.group(1)

    def args(src, macro):
        return [tuple(int(a) for a in m.split(",")[:4]) for m in re.findall(r"\b%s\s*\(([^()]*)\)" % macro, src)]

    out = set()
    for R, wgc, nj, by in args(body("kMarch"), "LES_MARCH_ENTRY"):
        out.add(("march", R, (wgc, nj, by)))
    for R, v, *_ in args(body("kStrips"), "LES_STRIP_ENTRY"):
        out.add(("strip", R, v))
    for a in args(body("kNaiveStrips"), "LES_NAIVE_ENTRY"):
        out.add(("naive", a[0], 0))
    m = re.search(r"#define\s+LES_INTERP_ENTRIES\s*\(\s*SRC_\s*\)(.*)", text)
    assert m, "LES_INTERP_ENTRIES not found"
    interp_radii = [int(r) for r in re.findall(r"\bLES_INTERP_ENTRY\s*\(\s*(\d+)\s*,", m.group(1))]
    for fam, arr in (("nearest", "kNearestStrips"), ("quadratic", "kQuadraticStrips")):
        b = body(arr)
        assert "LES_INTERP_ENTRIES" in b, arr
        for R in interp_radii * b.count("LES_INTERP_ENTRIES"):
            out.add((fam, R, 0))
    return out


# ------------------------------------------------------------------------------------------------ job cuts
@contextlib.contextmanager
def env(**kv):
    """Set (value) or unset (None) environment variables for the body (the library reads them with getenv)."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def groups(trs, R, entry, rows):
    """Workgroups of build_march_jobs' cut: entry ("wide" / "narrow"), rows per job."""
    wgc, nj = MARCH_ENTRIES[entry]
    TW = wgc - 4 * R
    n = 0
    for t in np.asarray(trs).reshape(-1):
        tw, th = int(t["w"]), int(t["h"])
        if tw <= 0 or th <= 0:
            continue
        ns = -(-tw // TW)
        sw = -(-tw // ns)
        nr = -(-th // rows)
        sh = -(-th // nr)
        n += -(-tw // sw) * -(-th // sh)
    return -(-n // nj)


def cuts(R):
    """(name, environment, entry or None, rows or None): the default, each entry at the cost model's rows, and rows 1, BY, BY + 1."""
    BY = MARCH_BY[R]
    out = [("default", {}, None, None)]
    for entry, w in (("wide", 1), ("narrow", 0)):
        out.append((entry, {"LES_HIP_MARCH_WIDE": w}, entry, None))
        for rows in (1, BY, BY + 1):
            out.append((f"{entry}-rows{rows}", {"LES_HIP_MARCH_WIDE": w, "LES_HIP_MARCH_ROWS": rows}, entry, rows))
    return out


def strip_jobs(trs, R, TW):
    """Jobs of build_jobs' cut for the strip kernel: TW-column strips, row chunks of at least max(8R, 64) rows when there are few strips."""
    ts = [(int(t["w"]), int(t["h"])) for t in np.asarray(trs).reshape(-1) if t["w"] > 0 and t["h"] > 0]
    strips = sum(-(-w // TW) for w, _ in ts)
    rows = 1 << 30
    if 0 < strips < 2048:
        want = -(-2048 // strips)
        rows = max(max(8 * R, 64), -(-max(h for _, h in ts) // want))
    return sum(-(-w // TW) * -(-h // rows) for w, h in ts)


def strip_tw(R, variant=0):
    """Output columns per strip job of the strip kernels of radius R (stage-1 columns WA - 2R; WA 64, 96 at radius 15, 128 for variant 8)."""
    return (128 if variant == 8 else 96 if R == 15 else 64) - 2 * R


def run_cut(e, frs, trs, planes, mode, check, out_slabs, R, cut, kind=1, tw=None):
    """One fresh batch under `cut`: kernel kind and workgroup count asserted (tw: strip width of a kind-0 batch), output downloaded
    ([slabs][H][W], FILL where unwritten)."""
    name, ev, entry, rows = cut
    frs, trs = api._rects(frs), api._rects(trs)
    with env(**{"LES_HIP_MARCH_WIDE": None, "LES_HIP_MARCH_ROWS": None, **{k: str(v) for k, v in ev.items()}}):
        b = api.Batch(e, frs, trs, out_slabs=out_slabs)
    n = len(frs)
    nslab = 1 if out_slabs == 0 else n // out_slabs
    buf = api.DeviceBuffer(e, nslab * e.H * e.W * 4)
    try:
        assert b.kernel_kind(mode) == kind, (name, b.kernel_kind(mode), kind)
        if kind == 1:
            if entry is None:
                want = {groups(trs, R, en, ro) for en in MARCH_ENTRIES for ro in ROW_OPTS}
            elif rows is None:
                want = {groups(trs, R, entry, ro) for ro in ROW_OPTS}
            else:
                want = {groups(trs, R, entry, rows)}
            assert b.num_jobs in want, f"cut {name}: {b.num_jobs} workgroups, expected one of {sorted(want)}"
        elif kind == 0 and tw is not None:
            assert b.num_jobs == strip_jobs(trs, R, tw), (b.num_jobs, strip_jobs(trs, R, tw))
        out = np.full((nslab, e.H, e.W), ic.FILL, F32)
        buf.upload(out)
        b.run(planes, buf.ptr, mode=mode, check=check)
        e.synchronize()
        return buf.download((nslab, e.H, e.W), F32)
    finally:
        buf.free()
        b.destroy()


def run_all_cuts(e, frs, trs, planes, mode, check, out_slabs, R, which=None, kind=1):
    """The batch under every cut of `which` (default: all): the outputs must be bit-identical; returns the default cut's."""
    outs = []
    for cut in cuts(R):
        if which is not None and cut[0] not in which:
            continue
        outs.append((cut[0], run_cut(e, frs, trs, planes, mode, check, out_slabs, R, cut, kind)))
    for name, o in outs[1:]:
        d = o.view(np.uint32) != outs[0][1].view(np.uint32)
        assert not d.any(), f"radius {R}: cut {name} differs from cut {outs[0][0]} at {int(d.sum())} pixels"
    return outs[0][1]


# ------------------------------------------------------------------------------------------------ comparisons that count
class Tally:
    """Worst error and number of compared pixels per (family, radius); every comparison asserts its own floor."""

    def __init__(self):
        self.rows = {}

    def add(self, key, err, n):
        w, c = self.rows.get(key, (0.0, 0))
        self.rows[key] = (max(w, err), c + n)

    def report(self):
        return "\n".join(f"{k[0]:>18} R={k[1]:<3} worst abs err {w:.2e}  finite px {c}" for k, (w, c) in sorted(self.rows.items()))


def finite_count(ref, written=None):
    ref = np.asarray(ref)
    v = ~np.isnan(ref) & (ref != float(SENT))
    if written is not None:
        v &= written
    return int(v.sum())


def oracle_compare(got, ref, min_px, tight=True):
    """pc.compare_maps (NaN = unwritten) plus the floor on compared pixels."""
    n = finite_count(ref)
    assert n >= min_px, f"only {n} finite, non-sentinel pixels compared (floor {min_px})"
    return pc.compare_maps(got, ref, tight=tight), n


def restated_compare(pr, got, ref, S, written, min_px):
    """interp_cases.compare (any filter; NaN a legitimate output) plus the floor on compared pixels."""
    n = finite_count(ref, written)
    assert n >= min_px, f"only {n} finite, non-sentinel pixels compared (floor {min_px})"
    assert np.all(got[~written] == ic.FILL), "pixels outside the targets were written"
    return ic.compare(pr, got, ref, S, written), n


def oracle_batch(o, frs, trs, planes, mode, check, out_slabs, H, W):
    """The oracle's output of a batch, [slabs][H][W] (NaN where nothing is written)."""
    frs, trs = api._rects(frs), api._rects(trs)
    n = len(frs)
    if out_slabs == 0:
        return o.unary_batch(frs, trs, planes, mode=mode, check=check)[None].astype(np.float64)
    ref = np.full((n // out_slabs, H, W), np.nan)
    for s in range(n // out_slabs):
        sl = slice(s * out_slabs, (s + 1) * out_slabs)
        ref[s] = o.unary_batch(frs[sl], trs[sl], planes[sl], mode=mode, check=check)
    return ref


def nan_unwritten(got, trs, out_slabs):
    """got with FILL replaced by NaN where no target lies (the oracle's convention); asserts nothing else holds FILL."""
    got = got.astype(np.float32).copy()
    written = np.zeros(got.shape, bool)
    for i, t in enumerate(np.asarray(api._rects(trs))):
        s = 0 if out_slabs == 0 else i // out_slabs
        written[s, t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]] = True
    assert np.all(got[~written] == ic.FILL), "pixels outside the targets were written"
    got[~written] = np.nan
    return got


# ------------------------------------------------------------------------------------------------ scenes and planes
def scene(H, W, D, seed=42):
    return synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235), synth.make_volume(D, H, W, seed), synth.make_volume(D, H, W, seed + 1)


def kind_planes(D, H, W):
    """Planes that reach role A's KIND 0 (integer fronto-parallel, clamped and invalid ones too), 1 (fractional fronto-parallel), 4 (short
    gather: slanted, finite), 5 (steep along x: the tiled copy) and 2 (NaN; every general plane of a context with min_disp != 0)."""
    cx, cy = W / 2.0, H / 2.0
    p = [(0.0, 0.0, 3.0), (0.0, 0.0, -1.0), (0.0, 0.0, D + 2.0), (0.0, 0.0, 2.5), (0.0, 0.0, D - 1.25),
         (0.02, -0.03, 0.0), (-0.04, 0.05, 0.0), (0.5, 0.1, 0.0), (-0.26, 0.0, 0.0), (0.06, -0.2, 0.0), (float("nan"), 0.1, 3.0)]
    out = np.zeros((len(p), 4), F32)
    for i, (a, b, c) in enumerate(p):
        zc = c if (a == 0.0 and b == 0.0) or np.isnan(a) else (D - 1) * (0.3 + 0.4 * ((i * 7) % 5) / 4.0)
        out[i] = (a, b, c if (a == 0.0 and b == 0.0) or np.isnan(a) else zc - a * cx - b * cy, 0.0)
    return out


def inner_planes(n, D, H, W, seed, margin=1.0):
    """Slanted planes whose disparity stays within [margin, D - 1 - margin] over the whole image (interpolation 2 values: no end slices)."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 4), F32)
    lo, hi = margin, D - 1 - margin
    for i in range(n):
        span = (hi - lo) * 0.8
        a = rng.uniform(-1, 1) * span / 2.0 / max(W, 1)
        b = rng.uniform(-1, 1) * span / 2.0 / max(H, 1)
        zc = (lo + hi) / 2.0 + rng.uniform(-0.1, 0.1) * span
        p[i] = (a, b, zc - a * (W - 1) / 2.0 - b * (H - 1) / 2.0, 0.0)
    p[0] = (0.0, 0.0, round((lo + hi) / 2.0), 0.0)
    p[1] = (0.0, 0.0, (lo + hi) / 2.0 + 0.375, 0.0)
    return p


def mixed_cell_planes(n, D, H, W, seed):
    """Planes inside the range (valid labels) with every third one drawn freely (often partly invalid)."""
    p = inner_planes(n, D, H, W, seed)
    p[2::3] = pc.random_planes(n, D, H, W, seed, slant=0.1)[2::3]
    return p


def v_planes(n, D, H, W, seed):
    """mixed_cell_planes with vertical disparities: fractional, integer, beyond a row, -0.0 and 0 (those keep the v = 0 bits)."""
    p = mixed_cell_planes(n, D, H, W, seed)
    p[:, 3] = np.resize(np.array([0.75, -1.0, 0.37, 2.5 + 1 / 64, -0.0, 0.0], F32), n)
    return p


def layer_cells(W, H, R, unit):
    layer = om.Layer(W, H, 2 * R, unit)
    cells = layer.sets[0]
    return layer.filter[cells], layer.shared[cells]


# ------------------------------------------------------------------------------------------------ march matrix
def case_march_volume(lib, R, H, W, D, tally, which=None):
    """Volume energy at interpolation 1 on the march kernel of radius R, against the oracle: whole-image slabs of kind_planes (both views,
    check 0 / 1) in contexts with min_disp 0 and -2 (KIND 2), and LayerManager cells, under every cut."""
    imL, imR, vL, vR = scene(H, W, D)
    for mind in (0.0, -2.0):
        pr = pc.Pair(lib, imL, imR, vL, vR, windR=2 * R, max_disp=D - 1 + mind, min_disp=mind)
        try:
            planes = kind_planes(D, H, W)
            planes[:, 2] += mind
            full = api._rects([(0, 0, W, H)] * len(planes))
            for mode, check in ((0, True), (1, False)) if mind == 0.0 else ((1, True),):
                got = run_all_cuts(pr.e, full, full, planes, mode, check, 1, R, which)
                ref = oracle_batch(pr.o, full, full, planes, mode, check, 1, H, W)
                err, n = oracle_compare(nan_unwritten(got, full, 1), ref, min_px=H * W * len(planes) // 3)
                tally.add(("march volume", R), err, n)
            if mind == 0.0:
                frs, trs = layer_cells(W, H, R, max(3, min(H, W) // 3))
                cp = mixed_cell_planes(len(frs), D, H, W, 7 + R)
                for mode, check in ((1, True), (0, False)):
                    got = run_all_cuts(pr.e, frs, trs, cp, mode, check, 0, R, which)
                    ref = oracle_batch(pr.o, frs, trs, cp, mode, check, 0, H, W)
                    err, n = oracle_compare(nan_unwritten(got, trs, 0), ref, min_px=int(trs["w"] @ trs["h"]) // 3)
                    tally.add(("march volume cells", R), err, n)
        finally:
            pr.close()


def case_march_interp(lib, R, H, W, D, tally, which=None):
    """Interpolation 0 and 2 on the march kernel of radius R (raw-cost pre-pass, KIND 3, at 2 the mv2 scale and the flagged calls recomputed
    on the strip kernel) against InterpPair.expected: values on planes at least one slice inside the range; calls on the end slices (all
    NaN at 2) flagged in the same batch and checked for their NaN sets."""
    imL, imR, vL, vR = scene(H, W, D)
    for interp in (0, 2):
        pr = ic.InterpPair(lib, imL, imR, vL, vR, interp, windR=2 * R)
        try:
            planes = inner_planes(6, D, H, W, 3 + R)
            full = api._rects([(0, 0, W, H)] * len(planes))
            for mode, check in ((0, True), (1, False)):
                got = run_all_cuts(pr.e, full, full, planes, mode, check, 1, R, which)
                ref, S, written = ic.expected_batch(pr, full, full, planes, mode, check, out_slabs=1)
                worst, count = 0.0, 0
                for s in range(len(planes)):
                    err, n = restated_compare(pr, got[s], ref[s], S[s], written[s], min_px=H * W // 2)
                    worst, count = max(worst, err), count + n
                tally.add((f"march interp{interp}", R), worst, count)
            # cells: a few clean planes, the others on slice 0 / D - 1 (flagged at interpolation 2: the strip kernel recomputes them)
            frs, trs = layer_cells(W, H, R, max(3, min(H, W) // 3))
            cp = inner_planes(len(frs), D, H, W, 11 + R)
            cp[1::3] = (0.0, 0.0, 0.0, 0.0)
            cp[2::3] = (0.0, 0.0, float(D - 1), 0.0)
            clean = np.ones(len(frs), bool)
            clean[1::3] = clean[2::3] = False
            got = run_all_cuts(pr.e, frs, trs, cp, 0, True, 0, R, which)[0]
            ref, S, written = ic.expected_batch(pr, frs, trs, cp, 0, True)
            ref, S, written = ref[0], S[0], written[0]
            inner = np.zeros_like(written)
            for t in np.asarray(api._rects(trs))[clean]:
                inner[t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]] = True
            err, n = restated_compare(pr, got, ref, S, written, min_px=0)
            assert finite_count(ref, inner) >= int(np.asarray(api._rects(trs))[clean]["w"] @ np.asarray(api._rects(trs))[clean]["h"]) // 2
            if interp == 2:
                ends = written & ~inner
                assert ends.any() and np.isnan(ref[ends]).all() and np.isnan(got[ends]).all(), "end-slice calls at interpolation 2 must be NaN"
            tally.add((f"march interp{interp} cells", R), err, finite_count(ref, inner))
        finally:
            pr.close()


def naive_pair(lib, R, H, W, filter="GF", max_disp=7.0, sig2=10.0, windR=None):
    imL, imR = synth.make_guide(H, W, 1234), synth.make_guide(H, W, 1235)
    return vc.VPair(lib, filter=filter, windR=2 * R if windR is None else windR, sig2=sig2, max_disp=max_disp, ims=(imL, imR))


def case_march_naive(lib, R, H, W, tally, which=None):
    """The image-based energy on the march kernel of radius R (pre-pass + KIND 3): v = 0 against the oracle, v != 0 against the vdisp_cases
    restatement, whole-image slabs and LayerManager cells."""
    pr = naive_pair(lib, R, H, W)
    try:
        planes = mixed_cell_planes(6, pr.D, H, W, 5 + R)
        planes[0] = (0.0, 0.0, 2.0, 0.0)
        full = api._rects([(0, 0, W, H)] * len(planes))
        frs, trs = layer_cells(W, H, R, max(3, min(H, W) // 3))
        cp = mixed_cell_planes(len(frs), pr.D, H, W, 9 + R)
        for mode, check in ((0, True), (1, False)):
            got = run_all_cuts(pr.e, full, full, planes, mode, check, 1, R, which)
            ref = oracle_batch(pr.o, full, full, planes, mode, check, 1, H, W)
            err, n = oracle_compare(nan_unwritten(got, full, 1), ref, min_px=H * W * len(planes) // 3, tight=pc.NAIVE_TIGHT)
            tally.add(("march image v=0", R), err, n)
            got = run_all_cuts(pr.e, frs, trs, cp, 1 - mode, check, 0, R, which)
            ref = oracle_batch(pr.o, frs, trs, cp, 1 - mode, check, 0, H, W)
            err, n = oracle_compare(nan_unwritten(got, trs, 0), ref, min_px=int(trs["w"] @ trs["h"]) // 3, tight=pc.NAIVE_TIGHT)
            tally.add(("march image v=0 cells", R), err, n)
        for (fr, tr, pl, slabs) in ((full, full, v_planes(len(full), pr.D, H, W, 13 + R), 1), (frs, trs, v_planes(len(frs), pr.D, H, W, 14 + R), 0)):
            got = run_all_cuts(pr.e, fr, tr, pl, 0, True, slabs, R, which)
            ref, S, written = ic.expected_batch(pr, fr, tr, pl, 0, True, out_slabs=slabs)
            count = 0
            for s in range(got.shape[0]):
                err, n = restated_compare(pr, got[s], ref[s], S[s], written[s], min_px=0)
                tally.add(("march image v!=0", R), err, n)
                count += n
            assert count >= int(written.sum()) // 3, f"only {count} finite, non-sentinel pixels compared"
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ strip matrix
def strip_calls(H, W, R, D):
    """A whole-image call and a call whose target hugs the left border of an inner filterRect (the strip kernel on any build)."""
    fr = (1, 0, W - 1, H)
    return [((0, 0, W, H), (0, 0, W, H)), (fr, (1, 0, max(1, (W - 1) // 2), H))]


def case_strip_family(lib, fam, R, H, W, D, tally, variant=None):
    """One strip-kernel family at radius R (contexts created with LES_HIP_KERNEL=strip; the border-hugging call would take it anyway):
    kernel kind 0 and parity with the family's reference."""
    with env(LES_HIP_KERNEL="strip", LES_HIP_VARIANT=variant):
        if fam == "strip":
            pr = pc.synth_pair(lib, H, W, D, windR=2 * R)
        elif fam in ("nearest", "quadratic"):
            imL, imR, vL, vR = scene(H, W, D)
            pr = ic.InterpPair(lib, imL, imR, vL, vR, 0 if fam == "nearest" else 2, windR=2 * R)
        else:
            pr = naive_pair(lib, R, H, W)
    try:
        calls = strip_calls(H, W, R, D)
        frs = api._rects([c[0] for c in calls] * 3)
        trs = api._rects([c[1] for c in calls] * 3)
        n = len(frs)
        if fam == "quadratic":
            pl = inner_planes(n, D, H, W, 17 + R)
            pl[-1] = (0.0, 0.0, float(D - 1), 0.0)            # end slice: NaN
        elif fam == "naive":
            pl = v_planes(n, pr.D, H, W, 19 + R)             # v != 0: recomputed on the nearest-slice strip kernel
        else:
            pl = mixed_cell_planes(n, D, H, W, 23 + R)
        for mode, check in ((0, True), (1, False)):
            got = run_cut(pr.e, frs, trs, pl, mode, check, 1, R, ("strip", {}, None, None), kind=0, tw=strip_tw(R, variant or 0))
            if fam == "strip":
                ref = oracle_batch(pr.o, frs, trs, pl, mode, check, 1, H, W)
                err, cnt = oracle_compare(nan_unwritten(got, trs, 1), ref, min_px=int(trs["w"] @ trs["h"]) // 3)
            else:
                ref, S, written = ic.expected_batch(pr, frs, trs, pl, mode, check, out_slabs=1)
                err, cnt = 0.0, 0
                for s in range(n):
                    e_, c_ = restated_compare(pr, got[s], ref[s], S[s], written[s], min_px=0)
                    err, cnt = max(err, e_), cnt + c_
                assert cnt >= int(written.sum()) // 3, f"only {cnt} finite, non-sentinel pixels compared"
                if fam == "quadratic":
                    assert np.isnan(got[n - 1][written[n - 1]]).all()
            tally.add((f"strip {fam}" + (f" v{variant}" if variant else ""), R), err, cnt)
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ shapes
def shapes(R):
    """Image shapes (H, W) that stress the job cut of radius R: thin, tiny, the window's size, and widths at both march entries' TW +- 1."""
    out = [(1, 37), (37, 1), (2, 2), (5, 7), (2 * R, 23), (2 * R + 1, 23), (9, 2 * R), (9, 2 * R + 1)]
    for wgc, _ in MARCH_ENTRIES.values():
        TW = wgc - 4 * R
        out += [(6, TW - 1), (6, TW), (6, TW + 1)]
    return out


def shape_pair(lib, H, W, D, filter, naive, R):
    imL, imR, vL, vR = scene(H, W, D)
    if filter == "GF":
        if naive:
            return pc.NaivePair(lib, imL, imR, float(D - 1), windR=2 * R)
        return pc.Pair(lib, imL, imR, vL, vR, windR=2 * R)
    if naive:
        return bc.BfPair(lib, imL, imR, naive=True, max_disp=float(D - 1), windR=R, sig2=10.0, filter=filter)
    return bc.BfPair(lib, imL, imR, vL, vR, windR=R, sig2=10.0, filter=filter, max_disp=float(D - 1))


def case_shape(lib, H, W, R, filter, naive, tally, strip=False, D=6):
    """Whole-image slabs (4 planes: NP 4 of the bilateral kernel), one single-plane slab (NP 1) and 1 x 1 targets at the four corners of a
    whole-image filterRect, both views, against the oracle (GF) or the bilateral / unfiltered restatement.  A GF context on the march kernel
    runs every batch with the wide and with the narrow entry forced too (bit-identical), so both entries meet their own TW boundary."""
    with env(LES_HIP_KERNEL="strip" if strip else None):
        pr = shape_pair(lib, H, W, D, filter, naive, R)
    try:
        full = (0, 0, W, H)
        pl = np.array([(0.0, 0.0, 2.0, 0.0), (0.0, 0.0, 1.5, 0.0), (0.1, -0.1, 2.0, 0.0), (-0.05, 0.02, 3.0, 0.0)], F32)
        corners = [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]
        batches = [([full] * 4, [full] * 4, pl, 1), ([full], [full], pl[2:3], 1), ([full] * 4, corners, pl, 1)]
        kind = 2 if filter != "GF" else None
        for bi, (frs, trs, planes, slabs) in enumerate(batches):
            frs, trs = api._rects(frs), api._rects(trs)
            mode, check = (bi % 2, bi != 1)
            with env(LES_HIP_MARCH_WIDE=None, LES_HIP_MARCH_ROWS=None):
                b = api.Batch(pr.e, frs, trs, out_slabs=slabs)
                k = b.kernel_kind(mode)
                b.destroy()
            if kind is not None:
                assert k == kind
            else:
                assert k == (0 if strip else 1), (k, strip)
            if k == 1:
                got = run_all_cuts(pr.e, frs, trs, planes, mode, check, slabs, R, which=("default", "wide", "narrow"))
            else:
                got = run_cut(pr.e, frs, trs, planes, mode, check, slabs, R, ("default", {}, None, None), kind=k)
            px = len(trs) * int(trs[0]["w"]) * int(trs[0]["h"])
            floor = max(1, px // 3)
            if filter == "GF":
                ref = oracle_batch(pr.o, frs, trs, planes, mode, check, slabs, H, W)
                err, n = oracle_compare(nan_unwritten(got, trs, slabs), ref, min_px=floor, tight=pc.NAIVE_TIGHT if naive else True)
            else:
                err, n = 0.0, 0
                for s, (f, t, p) in enumerate(zip(frs, trs, planes)):
                    ref, S = pr.expected(tuple(f), tuple(t), tuple(p), mode, check)
                    g = nan_unwritten(got[s:s + 1], trs[s:s + 1], 1)[0]
                    c = finite_count(ref)
                    err, n = max(err, bc.compare(g, ref, S, exact=pr.R == 0)), n + c
                assert n >= floor, f"only {n} finite pixels compared"
            tally.add((f"shape {filter or 'none'}{' image' if naive else ''}{' strip' if strip else ''}", R), err, n)
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ the plain build
def case_plain_vs_product(plain_lib, R, entry, H, W, D=12):
    """Product against libles_plain.so at radius R with the entry forced: volume slabs (kind_planes) at interpolation 1 and 2, cells, and the
    image-based energy (KIND 3, v = 0 and v != 0); every output bit-identical.  -> arrays compared"""
    cut = ("forced", {"LES_HIP_MARCH_WIDE": 1 if entry == "wide" else 0}, entry, None)
    imL, imR, vL, vR = scene(H, W, D)
    outs = {}
    for tag, lib in (("product", None), ("plain", plain_lib)):
        res = []
        e = api.HipCostVolumeEnergy(imL, imR, vL, vR, windR=2 * R, eps=1e-4, th_col=0.5, lib=lib)
        try:
            planes = kind_planes(D, H, W)
            full = [(0, 0, W, H)] * len(planes)
            frs, trs = layer_cells(W, H, R, 14)
            cp = pc.random_planes(len(frs), D, H, W, 3 + R, slant=0.1)
            for interp in (1, 2):
                e.setInterpolationMethod(interp)
                ip = planes if interp == 1 else np.concatenate([inner_planes(6, D, H, W, R), planes[:2]])
                for mode, check in ((0, True), (1, False)):
                    res.append(run_cut(e, full[:len(ip)], full[:len(ip)], ip, mode, check, 1, R, cut))
                    res.append(run_cut(e, frs, trs, cp, mode, check, 0, R, cut))
        finally:
            e.close()
        en = api.HipCostVolumeEnergy.naive(imL, imR, windR=2 * R, eps=1e-4, max_disp=float(D - 1), lib=lib)
        try:
            res.append(run_cut(en, frs, trs, v_planes(len(frs), D, H, W, 7 + R), 0, True, 0, R, cut))
            res.append(run_cut(en, full[:6], full[:6], v_planes(6, D, H, W, 8 + R), 1, False, 1, R, cut))
        finally:
            en.close()
        outs[tag] = res
    for i, (a, b) in enumerate(zip(outs["product"], outs["plain"])):
        d = a.view(np.uint32) != b.view(np.uint32)
        assert not d.any(), f"radius {R} {entry}: output {i}: {int(d.sum())} values differ between the assembly and the plain build"
    return len(outs["product"])
