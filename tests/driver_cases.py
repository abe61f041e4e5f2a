"""Cases of tests/test_driver.py: the entry points of stereo.FastGCStereo, MidV2 and MidV3 as one driver -- what two of them must agree on, and that
each closes what it made -- on the CPU simulator build and on the MI355X, on the cones crop of the driver cases (crossview_cases.driver: the
image-based energy; sgm_cases.driver: the cost-volume energy of its AD-Census volumes; the two layers of crossview_cases).

Tolerances: none.  The maps compared come from the same calls with the same arguments on the same context (wta_labels or sgm_labels, then
post_process(left, right, 1.5, omega)), and the kernels' own tests require bit-identical repeats: equality is exact.  The counts are integers."""
import numpy as np

from localexpstereo_amd import api, gc, pm, stereo
from tests import crossview_cases as cv
from tests import sgm_cases as sc


# ------------------------------------------------------------------------------------------------ 1. entry points agree
def case_entry_points_agree(lib, device, device_cuts):
    """run(0, (0, 1), 0, labeling=s) against wta((0, 1)) / sgm((0, 1), **sgm_params): the same raw maps of both views, the same post-processed left
    map; with post_process=False the returned map is the raw one."""
    st, e, keep = sc.driver(lib, device, device_cuts)
    st.sgm_params = dict(paths=4)                  # (not the default: both sides have to pass it on)
    try:
        for s in ("wta", "sgm"):
            lab_run, raw_run = st.run(0, (0, 1), 0, labeling=s)
            raws_run = dict(st.raw_labelings)
            st.raw_labelings = {}
            lab, raw = st.wta((0, 1)) if s == "wta" else st.sgm((0, 1), **st.sgm_params)
            assert sorted(st.raw_labelings) == sorted(raws_run) == [0, 1]
            for m in (0, 1):
                assert cv.same(st.raw_labelings[m], raws_run[m]), (s, m)
            assert cv.same(raw, raw_run) and cv.same(raw, raws_run[0]) and cv.same(lab, lab_run), s
            assert not cv.same(lab, raw), s                              # (the post-processing had something to do)
            lab, raw = st.wta((0, 1), post_process=False) if s == "wta" else st.sgm((0, 1), post_process=False, **st.sgm_params)
            assert cv.same(lab, st.raw_labelings[0]) and cv.same(raw, raws_run[0]), s
    finally:
        st.close()
        e.close()
        del keep


# ------------------------------------------------------------------------------------------------ 2. everything made is closed
class Counted:
    """Counts, per class, the objects whose __init__ returned and those whose close() ran (an object's first close: some close twice, or again
    when they are collected)."""

    def __init__(self, monkeypatch, *classes):
        self.created, self.closed = {c.__name__: 0 for c in classes}, {c.__name__: 0 for c in classes}
        for c in classes:
            self._patch(monkeypatch, c)

    def _patch(self, monkeypatch, c):
        init, close, me = c.__init__, c.close, self

        def counted_init(obj, *a, **k):
            init(obj, *a, **k)
            me.created[c.__name__] += 1
            obj._counted_open = True

        def counted_close(obj, *a, **k):
            if getattr(obj, "_counted_open", False):
                obj._counted_open = False
                me.closed[c.__name__] += 1
            return close(obj, *a, **k)
        monkeypatch.setattr(c, "__init__", counted_init)
        monkeypatch.setattr(c, "close", counted_close)

    def take(self):
        """-> (created, closed) since the last call"""
        out = dict(self.created), dict(self.closed)
        self.created, self.closed = {k: 0 for k in self.created}, {k: 0 for k in self.closed}
        return out


class Boom(RuntimeError):
    pass


def case_everything_closed(lib, device, device_cuts, monkeypatch):
    """After every entry point, whether it returns or raises: as many runners, graph-cut contexts and device evaluators closed as were made.
    -> {what: the numbers made}"""
    counts = Counted(monkeypatch, pm.PMRunner, gc.GraphCut, api.DeviceEvaluator)
    out = {}

    def check(what, made_at_least):
        created, closed = counts.take()
        assert created == closed, (what, created, closed)
        assert all(created[k] >= n for k, n in made_at_least.items()), (what, created)
        out[what] = created

    st, e = cv.driver(lib, device, device_cuts, evaluate_on_device=True, inner_loop_log=True)
    try:
        st.run(1, (0, 1), 1)
        check("run", dict(PMRunner=2, GraphCut=1, DeviceEvaluator=3))
        maps = {m: st.raw_labelings[m].copy() for m in (0, 1)}
        try:
            st.run(1, (0, 1), 0, labeling={0: maps[0]})
            raise AssertionError("a dict without view 1 was accepted")
        except ValueError as ex:
            assert "no map for view 1" in str(ex)
        check("run, the dict lacks view 1", dict(PMRunner=2, GraphCut=1, DeviceEvaluator=3))
        body, rows = stereo.FastGCStereo._evaluate_body, []

        def second_row_raises(self, index, mode, runner, g, t0):
            rows.append(index)
            if len(rows) == 2:
                raise Boom("second row")
            body(self, index, mode, runner, g, t0)
        with monkeypatch.context() as mp:
            mp.setattr(stereo.FastGCStereo, "_evaluate_body", second_row_raises)
            try:
                st.run(1, (0, 1), 1)
                raise AssertionError("the second row did not raise")
            except Boom:
                pass
        assert rows == [0, 1]
        check("run, the second row raises", dict(PMRunner=2, GraphCut=1, DeviceEvaluator=3))
        st.fuse(maps[0], [maps[0] * np.float32(0.5)])
        check("fuse", dict(PMRunner=1, GraphCut=1, DeviceEvaluator=1))
        st.cross_fuse(maps)
        check("cross_fuse", dict(PMRunner=2, GraphCut=1))
        st.wta((0, 1), slanted=True)
        check("wta(slanted=True)", dict(PMRunner=2, GraphCut=1, DeviceEvaluator=2))
    finally:
        st.close()
        e.close()
    # MidV2 whose run raises: the energy it made is closed
    made, closed = [], []
    naive, close = api.HipCostVolumeEnergy.naive, api.HipCostVolumeEnergy.close

    def counted_naive(*a, **k):
        made.append(naive(*a, **k))
        return made[-1]

    def counted_close(self):
        if self.h:
            closed.append(self)
        return close(self)

    def run_raises(self, *a, **k):
        raise Boom("run")
    monkeypatch.setattr(api.HipCostVolumeEnergy, "naive", staticmethod(counted_naive))
    monkeypatch.setattr(api.HipCostVolumeEnergy, "close", counted_close)
    monkeypatch.setattr(stereo.FastGCStereo, "run", run_raises)
    try:
        stereo.MidV2(cv.cones_data(), iterations=1, pmIterations=1, device=device, lib=lib, filterRadious=cv.WINDR)
        raise AssertionError("run did not raise")
    except Boom:
        pass
    assert len(made) == 1 and len(closed) == 1 and closed[0] is made[0], (len(made), len(closed))
    out["MidV2, run raises"] = dict(HipCostVolumeEnergy=len(made))
    return out
