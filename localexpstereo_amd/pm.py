"""Device-resident PatchMatch iterations of the local expansion loop, optionally sharded over the GPUs
of one node.

Reference loop: FastGCStereo::run / initCurrentFast / localExpansionMovesForLayer_CPU with doGC == false
(LES/FastGCStereo.h:22-72, 94-115, 133-169).  Cells of one disjoint set are independent
(LES/LayerManager.h:168-172), so every rank owns a contiguous band of the cells of each set, runs their
lock-steps (propose -> unary -> winner-take-all, all on the device through the C ABI) and then one
all-gather over RCCL/xGMI publishes the updated label/cost tiles of the set to every replica.  The
volume, the guide statistics and the label/cost maps are replicated; nothing is ever reduced.

torch is plumbing here: device buffers and torch.distributed (backend "nccl" == RCCL on ROCm, "gloo" for
the CPU tests that run against the simulator build of the same C ABI).
"""
import os
import time
from collections import Counter
from types import SimpleNamespace

import numpy as np
import torch

from . import api, gc as lgc


def layer_geometry(W, H, windR, unit):
    """LayerManager::addLayer geometry (LES/LayerManager.h:44-185) as numpy rect arrays + disjoint sets."""
    minsize = max(2, unit // 2)
    frac_w, frac_h = W % unit, H % unit
    split_w, split_h = frac_w >= minsize, frac_h >= minsize
    wb, hb = W // unit + int(split_w), H // unit + int(split_h)

    # (vectorised over the cells: the per-cell Python loop was 30 ms of a run's set-up at the Adirondack shape)
    def clip(x0, y0, x1, y1):
        x0, y0, x1, y1 = np.maximum(x0, 0), np.maximum(y0, 0), np.minimum(x1, W), np.minimum(y1, H)
        ok = (x1 > x0) & (y1 > y0)
        z = np.zeros_like(x0)
        return np.where(ok, x0, z), np.where(ok, y0, z), np.where(ok, x1 - x0, z), np.where(ok, y1 - y0, z)

    i, j = np.meshgrid(np.arange(hb, dtype=np.int64), np.arange(wb, dtype=np.int64), indexing="ij")
    i, j = i.reshape(-1), j.reshape(-1)
    ux1 = (j + 1) * unit + np.where((not split_w) & (j == wb - 1), frac_w, 0)
    uy1 = (i + 1) * unit + np.where((not split_h) & (i == hb - 1), frac_h, 0)
    units = np.stack(clip(j * unit, i * unit, ux1, uy1), axis=1)
    ex = np.where((not split_w) & (j == wb - 2), frac_w, 0)
    ey = np.where((not split_h) & (i == hb - 2), frac_h, 0)
    sx, sy, sw, sh = clip((j - 1) * unit, (i - 1) * unit, (j + 2) * unit, (i + 2) * unit)
    shared = np.stack([sx, sy, sw + ex, sh + ey], axis=1)
    fx, fy, fw, fh = clip((j - 1) * unit - windR, (i - 1) * unit - windR, (j + 2) * unit + windR, (i + 2) * unit + windR)
    filt = np.stack(clip(fx, fy, fx + fw + ex, fy + fh + ey), axis=1)
    phase = (i % 4) * 4 + (j % 4)
    cell = i * wb + j
    sets = [cell[phase == s] for s in range(16)]
    to = lambda a: np.array(a, np.int32).reshape(-1, 4).view(api.RECT_DT).reshape(-1)
    return to(units), to(shared), to(filt), [np.asarray(s, np.int64) for s in sets if len(s)]


def seeds_for(n, seed):
    """Non-zero 64-bit cv::RNG states, one per cell."""
    x = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(31)
    return np.where(x == 0, np.uint64(0xFFFFFFFF), x).astype(np.uint64)


class _Shard:
    """One (layer, disjoint set) on one rank: prepared batch of the rank's own cells + exchange indices."""

    def __init__(self, runner, units, shared, filt, cells, seeds, target_is_unit=False):
        e, dev = runner.e, runner.device
        world, rank = runner.world, runner.rank
        bounds = np.linspace(0, len(cells), world + 1).astype(int)          # contiguous bands of cells
        self.own = cells[bounds[rank]:bounds[rank + 1]]
        tgt = units if target_is_unit else shared
        self.n = len(self.own)
        self.regions = np.ascontiguousarray(tgt[self.own])
        self.batch_filter = np.ascontiguousarray(filt[self.own])
        self.batch = api.Batch(e, filt[self.own], tgt[self.own])
        self.batch.set_units(units[self.own])
        self.rng = torch.from_numpy(seeds[self.own].view(np.int64).copy()).to(dev)
        self.planes = torch.zeros((max(1, self.n), 4), dtype=torch.float32, device=dev)
        self.graph_off = self.batch.graph_offsets()
        self.graph_nodes = self.batch.graph_nodes()
        self.max_cell_nodes = self.batch.max_cell_nodes
        self.payload = self.payload_host = self.masks = self.masks_host = None      # views of the runner's staging buffers, cut on first use (_gc_buffers)
        # the plan of the set's tile exchange (C ABI: les_hip_exchange_*): every rank's target rects, this rank's slot layout
        self.xchg = api.Exchange(e, rank, [tgt[cells[bounds[r]:bounds[r + 1]]] for r in range(world)]) if world > 1 else None


def disparities(labels):
    """The disparity map of an H x W x 4 label map, on its device."""
    H, W = labels.shape[:2]
    ys, xs = torch.meshgrid(torch.arange(H, device=labels.device, dtype=torch.float32), torch.arange(W, device=labels.device, dtype=torch.float32), indexing="ij")
    return labels[..., 0] * xs + labels[..., 1] * ys + labels[..., 2]


class PMRunner:
    def __init__(self, energy, layer_units, proposer_table, seed=1, rank=0, world=1, device="cuda", mode=0, group=None, random_vdisp=None, device_cuts=None):
        """rank / world: this process's place among the ranks that share THIS view's cells; group: their torch.distributed process group
        (None = the default group).  Two-view runs on several ranks give each view its own group (stereo.FastGCStereo.run).
        random_vdisp: maxVDisp of the RANDOM proposals (RandomProposer(K, maxDisp, minDisp, maxVDisp)); None leaves the energy's setting."""
        self.e, self.rank, self.world, self.mode, self.group = energy, rank, world, mode, group
        if random_vdisp is not None:
            energy.set_random_vdisparity(random_vdisp)
        self.device = torch.device(device)
        if self.device.type == "cuda":
            # the torch ops of this class (exchange index_copy_, label / mask copies) run on torch's current stream: bind the
            # library's launches to the same stream so that their order is the program order under any stream context
            energy.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        self.H, self.W = energy.H, energy.W
        self.table = proposer_table
        self.maxd, self.mind = float(energy.max_disp), float(energy.params.min_disparity)
        windR = energy.params.windR
        self.labels = torch.zeros((self.H, self.W, 4), dtype=torch.float32, device=self.device)
        self.cur = torch.zeros((self.H, self.W), dtype=torch.float32, device=self.device)
        self.prop = torch.zeros((self.H, self.W), dtype=torch.float32, device=self.device)
        self.shards, self.init = [], None
        for li, unit in enumerate(layer_units):
            units, shared, filt, sets = layer_geometry(self.W, self.H, windR, unit)
            seeds = seeds_for(len(units), seed + 1000 * li)
            self.shards.append([_Shard(self, units, shared, filt, cells, seeds) for cells in sets])
            if li == 0:
                x0 = np.maximum(units["x"] - windR, 0); y0 = np.maximum(units["y"] - windR, 0)
                x1 = np.minimum(units["x"] + units["w"] + windR, self.W); y1 = np.minimum(units["y"] + units["h"] + windR, self.H)
                fr = np.stack([x0, y0, x1 - x0, y1 - y0], 1).astype(np.int32).view(api.RECT_DT).reshape(-1)
                self.init = _Shard(self, units, shared, fr, np.arange(len(units)), seeds_for(len(units), seed + 777), target_is_unit=True)
        self.sets = [(li, sh) for li, layer in enumerate(self.shards) for sh in layer]      # every (layer, shard of a disjoint set), in the order they are visited
        self.set_index = [k for layer in self.shards for k in range(len(layer))]            # ... and each one's number within its layer
        # the reference's doInnerLoopLog (LES/FastGCStereo.h:20,65): None, or a record (evaluator = api.DeviceEvaluator, params = the pairwise
        # parameters, meta = []) the driver sets: after every disjoint set one evaluation of this view's maps is ENQUEUED (no synchronisation; the
        # driver reads the evaluator's rows once at the end) and (iteration, layer, set) is appended to meta.  inner_iteration: the row index the
        # driver gives the iteration that is running.
        self.inner_log, self.inner_iteration = None, 0
        self.bytes_exchanged = 0
        self.exchanges = 0                       # all-gathers issued
        self._xevents = []
        self._xbuf = None                        # send / receive slots of the tile exchange: single-rank runs never exchange
        # the two switches a caller may set between construction and begin_gc (device_cuts: or give it here)
        self.device_cuts = device_cuts           # None | True | False | "all" | "fine" | "none": see begin_gc, which replaces it by one of the three names
        self.speculative_sets_on_cpu = False     # tests: take _gc_set_without_round_trips on the simulator too
        # graph-cut state: set by begin_gc; the buffers are sized from all shards and allocated by the first lock-step that needs them
        # (runs without graph-cut iterations, or with every cut on the device, never do)
        self.gc, self.device_graph, self._gc_mode, self._prop_host, self._env = None, True, self.mode, None, None
        self.gc_max_gap, self.gc_seconds, self.tiled_lockstep_ms = 0.0, Counter(), {}
        self._gc_staging = self._gc_status = None      # _gc_buffers: graphs and masks of a lock-step, device + pinned host; _status: a word per cell
        self._gc_tiled_ws = None                 # _cut_on_device: scratch of the tiled solver (runs without coarse layers have none)
        self._gc_check = None                    # _checked_moves: region energies before / after and flows of a lock-step's cells
        self._gc_snap = self._gc_fail = None     # _gc_set_without_round_trips: roll-back copy of labels / costs, the failure word
        self._joint_staging, self._joint = None, {}      # gc_iteration_joint (first runner only): staging for the cells of all views, set index -> record
        self._dumped = dict(tiled=0, tiled_written=0, samples=0, worst=0.012)     # tooling dumps: lock-steps seen / files written / slowest host cut so far (s)

    # -- exchange: one all-gather of the updated tiles of a set (labels 16 B/px + cost 4 B/px).  Pack and unpack are kernels of the
    # library on the runner's stream; with the nccl backend the collective is enqueued on the same stream by torch, so nothing here
    # waits on the host (gloo works on host tensors: the simulator's "device" memory is host memory).
    def _exchange(self, sh):
        if self.world == 1:
            return
        import torch.distributed as dist
        x = sh.xchg
        if x.slot_floats == 0:
            return
        if self._xbuf is None or self._xbuf[0].numel() < x.slot_floats:
            n = max([x.slot_floats] + [s.xchg.slot_floats for s in [s_ for _, s_ in self.sets] + [self.init] if s.xchg])
            self._xbuf = (torch.zeros(n, dtype=torch.float32, device=self.device), torch.zeros(n * self.world, dtype=torch.float32, device=self.device))
        send, recv = self._xbuf[0][: x.slot_floats], self._xbuf[1][: x.slot_floats * self.world]
        ev = None
        if self.device.type == "cuda":           # device time of pack -> all-gather -> unpack on this rank's stream (summed by exchange_seconds())
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record(torch.cuda.current_stream(self.device))
        x.pack(self.labels.data_ptr(), self.cur.data_ptr(), send.data_ptr())
        if self.device.type != "cuda":
            self._sync()
        if send.is_cuda and dist.get_backend(self.group) == "gloo":
            # functional tests of the multi-rank path on a box with ONE GPU (bench.py: LES_BENCH_BACKEND=gloo): gloo moves host memory
            send_h, recv_h = send.cpu(), torch.empty(recv.shape, dtype=recv.dtype)
            dist.all_gather_into_tensor(recv_h, send_h, group=self.group)
            recv.copy_(recv_h)
        else:
            dist.all_gather_into_tensor(recv, send, group=self.group)
        self.bytes_exchanged += recv.numel() * 4
        self.exchanges += 1
        x.unpack(recv.data_ptr(), self.labels.data_ptr(), self.cur.data_ptr())
        if ev is not None:
            ev[1].record(torch.cuda.current_stream(self.device))
            self._xevents.append(ev)

    def exchange_seconds(self):
        """Device seconds this rank's stream spent in the tile exchanges so far (pack -> all-gather -> unpack, events around each): what separates the
        collective's share from the cuts' in a multi-GPU run.  Synchronises."""
        if self.device.type != "cuda" or not self._xevents:
            return 0.0
        torch.cuda.synchronize(self.device)
        return sum(a.elapsed_time(b) for a, b in self._xevents) * 1e-3

    def _sync(self):
        self.e.synchronize()

    def _log_set(self, i):
        """Inner-loop log: one device evaluation after set i of self.sets, enqueued on the runner's stream."""
        if self.inner_log is None:
            return
        lg = self.inner_log
        lg.evaluator.evaluate(self.labels.data_ptr(), self.cur.data_ptr(), mode=self.mode, index=len(lg.meta), **lg.params)
        lg.meta.append((self.inner_iteration, self.sets[i][0], self.set_index[i]))

    def energy(self, params):
        """PMStereoBase::computeCurrentEnergy (LES/PMStereoBase.h:263-270) of this view's device maps, computed on the device: (data, smooth) =
        (sum of the current costs, sum of the forward smoothness terms).  params: lambda_, th_smooth, omega, epsilon.  Synchronises."""
        ev = api.DeviceEvaluator(self.e, max_rows=1)
        try:
            ev.evaluate(self.labels.data_ptr(), self.cur.data_ptr(), mode=self.mode, index=0, lambda_=params["lambda_"], th_smooth=params["th_smooth"],
                        omega=params["omega"], epsilon=params["epsilon"])
            row = ev.rows()[0]
        finally:
            ev.close()
        return row["data"], row["smooth"]

    def init_labels(self):
        """initCurrentFast (LES/FastGCStereo.h:94-115): random label per layer-0 cell + its unit-region cost."""
        sh = self.init
        if sh.n:
            sh.batch.propose(api.PROPOSE_INIT, self.labels.data_ptr(), sh.rng.data_ptr(), sh.planes.data_ptr())
            sh.batch.run(sh.planes.data_ptr(), self.cur.data_ptr(), mode=self.mode, check=True, planes_on_device=True)
        self._sync()
        self._exchange(sh)

    def init_from_labels(self, labels, rows_per_launch=64):
        """The warm-start branch of initCurrentFast (LES/FastGCStereo.h:116-130, "very slow" on the CPU): start from a
        given H x W x 4 label map (a host array, or a float32 tensor on the runner's device); the current cost of every pixel is the unary cost of its own label, evaluated with
        a 1 x 1 target and the filter region pixel +- windR -- one dense device pass (les_hip_unary_labels).
        rows_per_launch: accepted for callers of the former per-band launches, ignored."""
        if torch.is_tensor(labels) and labels.device == self.labels.device and labels.dtype == torch.float32:
            lab = labels                         # a device map (stereo.FastGCStereo's labeling="wta") is copied on the device
        else:
            lab = torch.as_tensor(np.ascontiguousarray(labels, np.float32)).to(self.device)
        assert tuple(lab.shape) == (self.H, self.W, 4)
        self.labels.copy_(lab)
        self.recost()             # (every rank evaluates the whole map: replicated state, nothing to exchange)

    def recost(self):
        """Re-evaluate the cost map from the label map (after the labels were changed behind the optimiser's back, e.g. by the
        post-processing): cur[p] = unary cost of labels[p].  Synchronises."""
        self.e.unary_labels(self.labels.data_ptr(), self.cur.data_ptr(), mode=self.mode, check=True)
        self._sync()

    def _proposals(self, li, iteration):
        """(kind, m) of every lock-step of a set of layer li, in the order of the proposer table.  The RandomProposer stops once its
        perturbation is below 0.1 disparities (LES/Proposer.h:149-152)."""
        for kind, K in self.table[li]:
            for m in range(iteration, iteration + K):
                if kind == api.PROPOSE_RANDOM and (self.maxd - self.mind) * 0.5 ** (m + 1) < 0.1:
                    break
                yield kind, m

    def _propose(self, sh, kind, m):
        """What every lock-step starts with: one proposal plane per cell of the shard and its unary costs (into self.prop)."""
        sh.batch.propose(kind, self.labels.data_ptr(), sh.rng.data_ptr(), sh.planes.data_ptr(), m=m)
        sh.batch.run(sh.planes.data_ptr(), self.prop.data_ptr(), mode=self.mode, check=True, planes_on_device=True)

    def iteration(self, iteration):
        """One PatchMatch iteration over all layers (LES/FastGCStereo.h:143-157 with doGC == false)."""
        for i, (li, sh) in enumerate(self.sets):
            for kind, m in self._proposals(li, iteration) if sh.n else ():
                self._propose(sh, kind, m)
                sh.batch.wta(sh.planes.data_ptr(), self.cur.data_ptr(), self.prop.data_ptr(), self.labels.data_ptr())
            if self.world == 1 or self.device.type != "cuda":
                self._sync()                     # (bounds the launch queue; with several ranks on GPUs the collective orders the stream itself)
            self._exchange(sh)
            self._log_set(i)

    # -- graph-cut iterations (LES/FastGCStereo.h:171-185: the main loop, doGC == true) ----------------------------
    # Proposals and unary costs come from the GPU exactly as in iteration(); the winner-take-all update is replaced by
    # the local expansion moves of the rank's own cells, cut on the device or on the host cores (gc.py).  Cross-rank coherence is the same
    # per-set all-gather.  One lock-step is: _propose, _graph, _cut (_cut_on_device, else _cut_on_host), _apply.  The cut steps take WHAT
    # is cut as a record (batch, n, regions, graph_off, graph_nodes, max_cell_nodes, payload / masks on the device and pinned on the
    # host): a _Shard, or the cells of two views as one batch (_joint_set).
    def begin_gc(self, graph_cut, mode=None, device_graph=True):
        """device_graph (default): the solution stays on the GPU -- pairwise terms / graph capacities of every move are
        computed there (les_hip_batch_expansion_graph), the host receives only the graphs, runs the max-flows and
        returns one mask byte per node, which the GPU applies (les_hip_batch_apply_masks).  False (or check=True in
        gc_iteration) = the reference's shape: host-resident solution, host graph construction."""
        self.gc = graph_cut
        self.device_graph = device_graph
        # device_cuts: cells small enough for a workgroup's LDS (the finest layer) are also CUT on the GPU (les_hip_batch_solve_graphs),
        # so neither their graphs nor their masks cross PCIe and the host cores only see the larger cells.
        # "all" (default on a GPU): the larger cells as well, by the tiled solver (les_hip_batch_solve_graphs_tiled: graphs resident in device
        # memory, a workgroup per tile); "fine": only the cells that fit the LDS (rounds 2-4); "none": every cut on the host.
        dc = self.device_cuts
        if dc is None:
            dc = "all" if self.device.type == "cuda" else "none"     # (the simulator build used by the CPU tests would spend minutes in it)
        elif dc is True:
            dc = "all"
        elif dc is False:
            dc = "none"
        if dc not in ("all", "fine", "none"):
            raise ValueError(f"device_cuts: {dc!r} (all | fine | none)")
        self.device_cuts = dc
        self._gc_mode = self.mode if mode is None else mode
        self.sync_gc_state()
        self._prop_host = self._pin(torch.empty((self.H, self.W), dtype=torch.float32))
        self.gc_max_gap = 0.0
        self.tiled_lockstep_ms = {}              # layer -> [(ms, launches)] of every lock-step the tiled solver cut (per view: a runner is a view)
        self.gc_seconds = Counter({"device": 0.0, "host_cuts": 0.0, "h2d": 0.0})      # (the other keys appear once they count something)
        self.gc_seconds.update({f"host_cuts_layer{li}": 0.0 for li in range(len(self.shards))})
        # the tooling's environment (what each variable does: _dump_host_cut, _dump_tiled, _gc_set_without_round_trips), read here and nowhere else
        env = os.environ.get
        self._env = SimpleNamespace(graphs=env("LES_DUMP_GRAPHS"), tiled=env("LES_DUMP_TILED"), every=env("LES_DUMP_EVERY"), full=env("LES_DUMP_FULL"),
                                    max=int(env("LES_DUMP_MAX", "6")), this_view=env("LES_DUMP_VIEW", str(self.mode)) == str(self.mode),
                                    per_lockstep=env("LES_GC_PER_LOCKSTEP_CHECK"))

    def sync_gc_state(self):
        """Copy the device solution into the host graph-cut context (for its energy queries / the host-construction path)."""
        m = self._gc_mode
        self._sync()
        self.gc.labels[m][...] = self.labels.cpu().numpy()
        self.gc.costs[m][...] = self.cur.cpu().numpy()

    def _pin(self, t):
        return t.pin_memory() if self.device.type == "cuda" else t

    def _staging(self, nodes):
        """Graph (5 floats per node) and mask (a byte per node) staging: device, pinned host, device, pinned host."""
        return (torch.empty(nodes * 5, dtype=torch.float32, device=self.device), self._pin(torch.empty(nodes * 5, dtype=torch.float32)),
                torch.empty(nodes, dtype=torch.uint8, device=self.device), self._pin(torch.zeros(nodes, dtype=torch.uint8)))

    @staticmethod
    def _stage(lk, staging):
        """Gives a lock-step record its views of a staging allocation, cut to its node count."""
        payload, payload_host, masks, masks_host = staging
        n = max(1, lk.graph_nodes)
        lk.payload, lk.payload_host, lk.masks, lk.masks_host = payload[: n * 5], payload_host[: n * 5], masks[:n], masks_host[:n]

    def _gc_buffers(self, sh):
        """Views of the runner-wide graph / mask staging buffers (one device + one pinned host allocation, sized for the
        largest lock-step) cut to this shard's node count."""
        if self._gc_staging is None:
            self._gc_staging = self._staging(max([1] + [s.graph_nodes for _, s in self.sets]))
        if sh.payload is None:
            self._stage(sh, self._gc_staging)

    def _status(self, n):
        """n of the runner's status words (int32 per cell, 0 = cut on the device): sized for its largest set; the joint batch of two views grows it."""
        if self._gc_status is None or self._gc_status.numel() < n:
            self._gc_status = torch.zeros(max([n] + [s.n for _, s in self.sets]), dtype=torch.int32, device=self.device)
        return self._gc_status[:n]

    def _graph(self, sh, payload_ptr):
        """The expansion graphs of the shard's cells (current labels against the proposals of _propose) into device memory at payload_ptr."""
        p = self.gc.params
        sh.batch.expansion_graph(sh.planes.data_ptr(), self.labels.data_ptr(), self.cur.data_ptr(), self.prop.data_ptr(), payload_ptr, mode=self.mode,
                                 lambda_=p["lambda_"], th_smooth=p["th_smooth"], omega=p["omega"], epsilon=p["epsilon"])

    def _apply(self, sh, masks_ptr):
        sh.batch.apply_masks(sh.planes.data_ptr(), masks_ptr, self.cur.data_ptr(), self.prop.data_ptr(), self.labels.data_ptr())

    def _on_device(self, lk):
        """Does the device try to cut this lock-step?"""
        return bool(lk.n) and (self.device_cuts == "all" or (self.device_cuts == "fine" and lk.max_cell_nodes <= api.Batch.MAXFLOW_MAX_NODES))

    def _cut_on_device(self, lk, li=None, iteration=None, flows=None):
        """Cuts the graphs at lk.payload into lk.masks: one workgroup per cell where every cell fits the LDS, else the tiled solver.  -> True: every
        cell was cut (else the status words say which were not).  li, iteration: where the lock-step belongs, for the per-layer statistics of the
        tiled solver and LES_DUMP_TILED (the joint form keeps neither).  flows: a float64 device tensor that receives every cell's flow through
        its n-links (the device self-check), or None."""
        st = self._status(lk.n)
        fp = flows.data_ptr() if flows is not None else None
        if lk.max_cell_nodes <= api.Batch.MAXFLOW_MAX_NODES:
            lk.batch.solve_graphs(lk.payload.data_ptr(), lk.masks.data_ptr(), st.data_ptr(), flows_dev=fp)
            done = not bool(st.any().item())         # (the only synchronisation of the lock-step)
        else:
            need = lk.batch.tiled_workspace_bytes() + 256
            if self._gc_tiled_ws is None or self._gc_tiled_ws.numel() < need:     # one scratch per runner (= per view and host thread), for its largest batch
                own = [s.batch.tiled_workspace_bytes() + 256 for _, s in self.sets if s.n and s.max_cell_nodes > api.Batch.MAXFLOW_MAX_NODES]
                self._gc_tiled_ws = torch.empty(max([need] + own), dtype=torch.uint8, device=self.device)
            ws, sec = self._gc_tiled_ws, self.gc_seconds
            wp = (ws.data_ptr() + 255) & ~255        # (the solver wants 256-byte alignment)
            t0 = time.perf_counter()
            nl = lk.batch.solve_graphs_tiled(lk.payload.data_ptr(), lk.masks.data_ptr(), st.data_ptr(), wp, ws.numel() - (wp - ws.data_ptr()), flows_dev=fp)
            sec["tiled_launches"] += nl
            sec["tiled_locksteps"] += 1
            if li is not None:
                handed = lk.batch.tiled_stats        # cells the host cores finished from their residual graphs (hand-over)
                sec["tiled_handed_cells"] += handed["handed_cells"]
                sec["tiled_handed_locksteps"] += 1 if handed["handed_cells"] else 0
                sec["tiled_handed_host_seconds"] += 1e-3 * handed["host_ms"]
                sec[f"tiled_seconds_layer{li}"] += time.perf_counter() - t0
                self.tiled_lockstep_ms.setdefault(li, []).append((1e3 * (time.perf_counter() - t0), nl))      # (wall of the solve call, launches enqueued)
                self._dump_tiled(lk, iteration, li, 1e3 * (time.perf_counter() - t0), nl)
            done = lk.batch.tiled_unsolved == 0      # (the call synchronised; it reports "cells that gave up" through a host-mapped word: no copy)
        if done:
            self.gc_seconds["cells_cut_on_device"] += lk.n
        return done

    def _cut_on_host(self, lk, nthreads, partial, flows=None):
        """Copies the graphs down, cuts them on the host cores, copies the masks up.  partial: when the device tried and gave up on only SOME
        cells (their status word is non-zero), only those are cut again and the device's masks of the others stay.  flows: as _cut_on_device
        (the cells cut here get the host solver's flow).
        -> (t1, t2): the clock before and after the cuts proper."""
        self._sync()
        lk.payload_host.copy_(lk.payload)
        regions, offsets = lk.regions, lk.graph_off
        failed = np.nonzero(self._status(lk.n).cpu().numpy())[0] if partial and self._on_device(lk) else ()
        t1 = time.perf_counter()
        if 0 < len(failed) < lk.n:
            lk.masks_host.copy_(lk.masks)
            regions, offsets = np.ascontiguousarray(regions[failed]), np.ascontiguousarray(offsets[failed])
            self.gc_seconds["cells_recut_on_host"] += len(failed)
        fh = np.zeros(len(regions), np.float64) if flows is not None else None
        lgc.solve_prebuilt(regions, lk.payload_host.numpy(), offsets, lk.masks_host.numpy(), nthreads=nthreads, flows_out=fh)
        t2 = time.perf_counter()
        lk.masks.copy_(lk.masks_host)
        if flows is not None:
            fd = torch.from_numpy(fh).to(self.device)
            if len(regions) < lk.n:
                flows[torch.from_numpy(np.asarray(failed, np.int64)).to(self.device)] = fd
            else:
                flows[: lk.n] = fd
        return t1, t2

    def _cut(self, lk, nthreads, partial, li=None, iteration=None, flows=None):
        """The cuts of a lock-step: on the device where device_cuts says so, on the host where not or when the device gave up.
        -> (every cell cut on the device, t1, t2): the clock before and after the host's cuts."""
        if self._on_device(lk) and self._cut_on_device(lk, li, iteration, flows):
            t = time.perf_counter()
            return True, t, t
        return (False,) + self._cut_on_host(lk, nthreads, partial, flows)

    def _moves_on_host_maps(self, sh, nthreads, check):
        """The lock-step in the reference's shape (check=True or device_graph=False): the proposals' costs go to the host, gc.expansion_moves builds
        and cuts the graphs there on the host-resident solution (with the reference's flow == energy self-check when `check`), and the fused maps
        come back.  -> (t1, t2) as _cut_on_host."""
        self._sync()
        self.gc_seconds["host_graph_locksteps"] += 1
        self._prop_host.copy_(self.prop)
        planes = sh.planes[: sh.n].cpu().numpy()
        t1 = time.perf_counter()
        gap = self.gc.expansion_moves(sh.regions, planes, self._prop_host.numpy(), mode=self.mode, nthreads=nthreads, check=check)
        self.gc_max_gap = max(self.gc_max_gap, gap)
        t2 = time.perf_counter()
        self.labels.copy_(torch.from_numpy(self.gc.labels[self.mode]))
        self.cur.copy_(torch.from_numpy(self.gc.costs[self.mode]))
        return t1, t2

    def _region_energy(self, sh, out):
        p = self.gc.params
        sh.batch.region_energy(self.labels.data_ptr(), self.cur.data_ptr(), out.data_ptr(), mode=self.mode, lambda_=p["lambda_"], th_smooth=p["th_smooth"],
                               omega=p["omega"], epsilon=p["epsilon"])

    def _checked_moves(self, sh, li, iteration, nthreads):
        """One lock-step on the device path with the reference's flow == energy self-check (LES/FastGCStereo.h:561-594) kept on the device: the graphs
        with their t-link flow, the cuts with their flow values, the energy of every cell's region before and after the masks are applied
        (les_hip_batch_region_energy).  Per cell gap = |flow0 + flow - E_after| / max(1, |E_after|), the host route's formula (host/les_gc.cpp);
        gc_max_gap is the largest; gc_seconds["moves_raised"] counts the cells whose move raised the energy by more than 1e-5 max(1, |E_after|).
        Cells the device hands to the host solver are checked with that solver's flow.  A diagnostic mode: it synchronises.
        gc_seconds["own_max_gap_<solver>"] keeps every device solver's own worst gap, gc_seconds["locksteps_checked_<solver>"] how many lock-steps
        each one cut (cell_kernel, lds_1024, lds_512: the most general one-workgroup kernel of the lock-step; tiled).  -> (t1, t2) as _cut_on_host."""
        p, n, sec = self.gc.params, sh.n, self.gc_seconds
        if self._gc_check is None or self._gc_check.shape[1] < n:
            self._gc_check = torch.zeros((3, max([n] + [s.n for _, s in self.sets])), dtype=torch.float64, device=self.device)
        e_before, e_after, flows = (self._gc_check[k, :n] for k in range(3))
        self._region_energy(sh, e_before)
        flow0 = sh.batch.expansion_graph(sh.planes.data_ptr(), self.labels.data_ptr(), self.cur.data_ptr(), self.prop.data_ptr(), sh.payload.data_ptr(),
                                         mode=self.mode, lambda_=p["lambda_"], th_smooth=p["th_smooth"], omega=p["omega"], epsilon=p["epsilon"], want_flow0=True)
        _, t1, t2 = self._cut(sh, nthreads, True, li, iteration, flows=flows)
        self._apply(sh, sh.masks.data_ptr())
        self._region_energy(sh, e_after)
        self._sync()
        eb, ea, fl = (t.cpu().numpy() for t in (e_before, e_after, flows))
        scale = np.maximum(1.0, np.abs(ea))
        gap = np.abs(flow0 + fl - ea) / scale
        if self._on_device(sh):
            # the device solvers push float residuals: next to the 1e6 terminals of invalid labels a push rounds at 0.06, and the tiled solver adds its
            # flow in fixed-point units, so a solver's own flow VALUE can be coarser than 1e-5 although its mask is a minimum cut.  Where it is, the
            # lock-step is checked against the host solver's flow on the same graphs (the value of a minimum cut does not depend on who computes
            # it); the solver's own worst gap is kept per kind.
            kind = "tiled" if sh.max_cell_nodes > api.Batch.MAXFLOW_MAX_NODES else ("cell_kernel", "lds_1024", "lds_512")[max(0, sh.batch.graph_solver_kind)]
            sec[f"own_max_gap_{kind}"] = max(sec[f"own_max_gap_{kind}"], float(np.max(np.where(np.isnan(gap), np.inf, gap))) if n else 0.0)
            sec[f"locksteps_checked_{kind}"] += 1
            if not np.all(gap <= 1e-5):
                th = time.perf_counter()
                sh.payload_host.copy_(sh.payload)
                fh, scratch = np.zeros(n, np.float64), np.zeros(max(1, sh.graph_nodes), np.uint8)
                lgc.solve_prebuilt(sh.regions, sh.payload_host.numpy(), sh.graph_off, scratch, nthreads=nthreads, flows_out=fh)
                gap = np.abs(flow0 + fh - ea) / scale
                sec["locksteps_checked_with_host_flow"] += 1
                sec["check_host_flow_seconds"] += time.perf_counter() - th      # (the check's own re-solve, not a cut of the run: host_cuts stays 0)
        worst = float(np.max(np.where(np.isnan(gap), np.inf, gap))) if n else 0.0
        self.gc_max_gap = max(self.gc_max_gap, worst)
        sec["moves_raised"] += int(np.count_nonzero(ea > eb + 1e-5 * scale))
        sec["cells_checked_on_device"] += n
        return t1, t2

    def _book(self, li, t0, t1, t2):
        """A lock-step's wall time: device work (and the way down) | the host cores' cuts | the way back up and the mask updates."""
        self.gc_seconds["device"] += t1 - t0
        self.gc_seconds["host_cuts"] += t2 - t1
        self.gc_seconds[f"host_cuts_layer{li}"] += t2 - t1
        self.gc_seconds["h2d"] += time.perf_counter() - t2

    def _dump_tiled(self, sh, iteration, li, ms, launches):
        """Tooling (tools/tiled_cut_replay.py): LES_DUMP_TILED=dir LES_DUMP_EVERY=n [LES_DUMP_VIEW=v LES_DUMP_MAX=k] writes the graphs of every
        n-th lock-step the tiled solver cut (regions, node offsets, the 5-float payload) with its wall time and launch count."""
        env, seen = self._env, self._dumped
        if not env.tiled or not env.this_view:
            return
        seen["tiled"] += 1
        if seen["tiled"] % int(env.every or "50") or seen["tiled_written"] >= env.max:
            return
        seen["tiled_written"] += 1
        np.savez_compressed(os.path.join(env.tiled, f"tiled_view{self.mode}_it{iteration}_layer{li}_{seen['tiled']}.npz"), regions=sh.regions, offsets=sh.graph_off,
                            payload=sh.payload[: sh.graph_nodes * 5].cpu().numpy(), ms=ms, launches=launches, cells=sh.n)

    def _dump_host_cut(self, sh, li, iteration, kind, it, on_dev, seconds):
        """Tooling (tools/cut_replay.py, tools/tiled_cut_replay.py), LES_DUMP_GRAPHS=dir: a timing log of the lock-steps; with LES_DUMP_EVERY=n a sample of
        ordinary ones (the first two cells, or with LES_DUMP_FULL all, of every n-th lock-step that was cut on the host); the graphs of the slowest
        lock-step of the coarsest layer."""
        env, seen, m = self._env, self._dumped, self.mode
        if not env.graphs:
            return
        with open(os.path.join(env.graphs, f"cutlog_view{m}.txt"), "a") as f:
            f.write(f"{iteration} {li} {kind} {it} {sh.n} {seconds:.6f}\n")
        every = int(env.every or "0")
        if every and not on_dev and env.this_view:
            seen["samples"] += 1
            if seen["samples"] % every == 0:
                k2 = sh.n if env.full else min(2, sh.n)
                nn = int(sh.graph_off[k2 - 1] + int(sh.regions[k2 - 1]["w"]) * int(sh.regions[k2 - 1]["h"]))
                np.savez_compressed(os.path.join(env.graphs, f"sample_view{m}_it{iteration}_layer{li}_{seen['samples']}.npz"), regions=sh.regions[:k2],
                                    offsets=sh.graph_off[:k2], payload=sh.payload_host.numpy()[: nn * 5].copy(), seconds=seconds, cells=sh.n)
        if li == len(self.shards) - 1 and iteration >= 1 and seconds > seen["worst"]:
            seen["worst"] = seconds
            np.savez_compressed(os.path.join(env.graphs, f"graphs_view{m}_layer{li}.npz"), regions=sh.regions, offsets=sh.graph_off,
                                payload=sh.payload_host.numpy()[: sh.graph_nodes * 5].copy(), seconds=seconds)

    def _gc_set_without_round_trips(self, sh, li, iteration):
        """All proposals of one disjoint set of the FINEST layer (cells that fit a workgroup's LDS: propose -> unary costs -> graph -> cut -> apply, nine
        times) enqueued without a single host round trip; the cuts count the cells that hit their iteration limit in ONE device word, read once at the
        end of the set (rounds 2-5 read a status word per lock-step: 720 synchronisations per view).  In the -- so far unobserved -- case that the word
        is not zero the set is rolled back (labels, costs, generator states were saved in device memory: 30 MB, microseconds) and the caller repeats it
        lock-step by lock-step with the host fall-back.  -> True: done."""
        if self.device.type != "cuda" and not self.speculative_sets_on_cpu:      # (the simulator would spend minutes in the cuts: only the test of this form)
            return False
        if self.device_cuts not in ("all", "fine") or sh.max_cell_nodes > api.Batch.MAXFLOW_MAX_NODES:
            return False
        if self._env.graphs or self._env.per_lockstep:       # (LES_DUMP_GRAPHS logs, LES_GC_PER_LOCKSTEP_CHECK=1 checks every lock-step)
            return False
        t0 = time.perf_counter()
        if self._gc_snap is None:
            self._gc_snap = (torch.empty_like(self.labels), torch.empty_like(self.cur))
            self._gc_fail = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._gc_buffers(sh)
        self._gc_snap[0].copy_(self.labels)
        self._gc_snap[1].copy_(self.cur)
        rng0 = sh.rng.clone()
        self._gc_fail.zero_()
        st, proposals = self._status(sh.n), list(self._proposals(li, iteration))
        for kind, m in proposals:
            self._propose(sh, kind, m)
            self._graph(sh, sh.payload.data_ptr())
            sh.batch.solve_graphs(sh.payload.data_ptr(), sh.masks.data_ptr(), st.data_ptr(), unsolved_total_dev=self._gc_fail.data_ptr())
            self._apply(sh, sh.masks.data_ptr())
        failed = int(self._gc_fail.item())                 # the set's only synchronisation
        self.gc_seconds["device"] += time.perf_counter() - t0
        if failed:
            self.labels.copy_(self._gc_snap[0])
            self.cur.copy_(self._gc_snap[1])
            sh.rng.copy_(rng0)
            self.gc_seconds["sets_rolled_back"] += 1
            return False
        self.gc_seconds["cells_cut_on_device"] += sh.n * len(proposals)
        self.gc_seconds["sets_without_round_trips"] += 1
        return True

    def gc_iteration(self, iteration, check=False, nthreads=0):
        """One graph-cut iteration of this view over all layers and sets."""
        device_check = check == "device"         # the self-check on the device path (_checked_moves); True: the reference's shape, on the host
        if device_check and not self.device_graph:
            raise ValueError('check="device" needs device-built graphs (begin_gc(device_graph=True))')
        host_maps = (bool(check) and not device_check) or not self.device_graph
        if host_maps:
            self.sync_gc_state()
        for i, (li, sh) in enumerate(self.sets):
            per_lock_step = sh.n and (host_maps or device_check or not self._gc_set_without_round_trips(sh, li, iteration))
            for kind, m in self._proposals(li, iteration) if per_lock_step else ():
                t0 = time.perf_counter()
                self._propose(sh, kind, m)
                if host_maps:
                    t1, t2 = self._moves_on_host_maps(sh, nthreads, bool(check))
                elif device_check:
                    self._gc_buffers(sh)
                    t1, t2 = self._checked_moves(sh, li, iteration, nthreads)
                else:
                    self._gc_buffers(sh)
                    self._graph(sh, sh.payload.data_ptr())
                    on_dev, t1, t2 = self._cut(sh, nthreads, True, li, iteration)      # (partial recut allowed)
                    self._dump_host_cut(sh, li, iteration, kind, m - iteration, on_dev, t2 - t1)
                    self._apply(sh, sh.masks.data_ptr())
                self._book(li, t0, t1, t2)
            if self.world > 1:
                self._exchange(sh)
                if host_maps:
                    torch.from_numpy(self.gc.labels[self.mode]).copy_(self.labels)
                    torch.from_numpy(self.gc.costs[self.mode]).copy_(self.cur)
            self._log_set(i)
        self._sync()

    # -- fusion moves (LES/FastGCStereo.h:241-410; definition and the deviation from the reference: csrc/les_pairwise.h) -----------------
    def fuse(self, labels_b, layers=None, nthreads=0):
        """Fuses the current solution with a second labelling `labels_b` (H x W x 4; a host array, or a float32 tensor on the runner's device, which is
        read in place and must stay unchanged during the call) by graph cuts: after begin_gc, for every disjoint set of the
        chosen layers (None = all; else the layer indices) one lock-step of fusion moves -- the graphs of the set's cells from the two label maps
        (les_hip_batch_fusion_graph), the cuts of the graph-cut iterations (_cut: the device solvers chosen per cell, the host where device_cuts says
        so or the device gave up), the masks applied from the label map (les_hip_batch_apply_masks_labels), a row of the inner-loop log.  The unary
        cost of b's label at a pixel does not depend on the current map: ONE dense pass (les_hip_unary_labels) into self.prop serves the whole call.
        A move never raises the energy (up to the float rounding of the capacities); every pixel ends with its own label of the current map or of b.
        -> dict: cells moved, pixels_taken (mask bytes set, summed over the sets: a pixel counts in every set whose cut gives it to b, also when it
        carries b's label already), nonsubmodular_pairs truncated, pairs built, seconds (the whole call, synchronised), dense_seconds (the dense pass,
        synchronised).
        Single rank: world > 1 raises NotImplementedError (the sets' tiles would have to be exchanged after every set)."""
        if self.world > 1:
            raise NotImplementedError("PMRunner.fuse is single-rank: multi-rank fusion is not implemented")
        if self.gc is None:
            raise RuntimeError("PMRunner.fuse needs begin_gc(graph_cut) first")
        t0 = time.perf_counter()
        if (torch.is_tensor(labels_b) and labels_b.device == self.labels.device and labels_b.dtype == torch.float32 and labels_b.is_contiguous()
                and labels_b.data_ptr() != self.labels.data_ptr()):
            lab = labels_b                       # a device map (stereo.FastGCStereo's cross-view step: the other view's warped labels) is used as is
        else:                                    # (any other array or tensor: converted through numpy, as before)
            lab = torch.as_tensor(np.ascontiguousarray(labels_b, np.float32)).to(self.device)
        assert tuple(lab.shape) == (self.H, self.W, 4)
        self.e.unary_labels(lab.data_ptr(), self.prop.data_ptr(), mode=self.mode, check=True)
        self._sync()
        dense = time.perf_counter() - t0
        p = self.gc.params
        counts = torch.zeros(max([1] + [sh.n for _, sh in self.sets]), dtype=torch.int32, device=self.device)
        taken = torch.zeros((), dtype=torch.int64, device=self.device)
        truncated = torch.zeros((), dtype=torch.int64, device=self.device)
        cells = pairs = 0
        for i, (li, sh) in enumerate(self.sets):
            if layers is not None and li not in layers:
                continue
            if sh.n:
                ts = time.perf_counter()
                self._gc_buffers(sh)
                sh.batch.fusion_graph(lab.data_ptr(), self.labels.data_ptr(), self.cur.data_ptr(), self.prop.data_ptr(), sh.payload.data_ptr(), mode=self.mode,
                                      lambda_=p["lambda_"], th_smooth=p["th_smooth"], omega=p["omega"], epsilon=p["epsilon"], nonsubmodular_dev=counts.data_ptr())
                _, t1, t2 = self._cut(sh, nthreads, True, li)
                sh.batch.apply_masks_labels(lab.data_ptr(), sh.masks.data_ptr(), self.cur.data_ptr(), self.prop.data_ptr(), self.labels.data_ptr())
                taken += (sh.masks[: sh.graph_nodes] != 0).sum()
                truncated += counts[: sh.n].sum()
                cells += sh.n
                w, h = sh.regions["w"].astype(np.int64), sh.regions["h"].astype(np.int64)
                pairs += int(((w - 1) * h + w * (h - 1) + 2 * (w - 1) * (h - 1)).sum())
                self._book(li, ts, t1, t2)
            self._log_set(i)
        self._sync()
        return dict(cells=cells, pixels_taken=int(taken.item()), nonsubmodular_pairs=int(truncated.item()), pairs=pairs,
                    seconds=time.perf_counter() - t0, dense_seconds=dense)

    def _joint_set(self, runners, k):
        """Set k of every view as ONE record for the cut steps: a joint batch (the views' target rects one after the other) has exactly the node
        offsets of the concatenated payload, so the single-batch entry points serve it unchanged.  views: (runner, shard, first node) of
        the views that have cells in the set."""
        if self._joint_staging is None:
            self._joint_staging = self._staging(max([1] + [sum(r.sets[i][1].graph_nodes for r in runners) for i in range(len(self.sets))]))
        lk = self._joint.get(k)
        if lk is None:
            shs = [r.sets[k][1] for r in runners]
            base = np.cumsum([0] + [sh.graph_nodes for sh in shs])
            lk = self._joint[k] = SimpleNamespace(
                n=sum(sh.n for sh in shs), batch=None, regions=np.concatenate([sh.regions for sh in shs]), graph_nodes=int(base[-1]),
                graph_off=np.concatenate([sh.graph_off + int(b) for sh, b in zip(shs, base)]).astype(np.int64),
                max_cell_nodes=max([0] + [sh.max_cell_nodes for sh in shs if sh.n]), views=[(r, sh, int(b)) for r, sh, b in zip(runners, shs, base) if sh.n])
            self._stage(lk, self._joint_staging)
        if lk.batch is None and self._on_device(lk):
            lk.batch = api.Batch(self.e, np.concatenate([sh.batch_filter for _, sh, _ in lk.views]), lk.regions)
            assert lk.batch.graph_nodes() == lk.graph_nodes and np.array_equal(lk.batch.graph_offsets(), lk.graph_off)
        return lk

    @staticmethod
    def gc_iteration_joint(runners, iteration, nthreads=0):
        """Graph-cut iteration of SEVERAL views in lock-step (two-view runs, LES/FastGCStereo.h:172-185: the views are independent
        until the post-processing).  Every lock-step evaluates the proposals of all views on the GPU and cuts the cells of all views at
        once: ONE solve on the device, or ONE payload to the host and ONE OpenMP team (twice the cells per fork/join, and for the coarsest
        layer twice the otherwise scarce parallelism); the masks are applied per view.  Same results as gc_iteration per view: the cuts of
        different views touch disjoint state.  Single rank, device-built graphs.  The counters are booked on the first runner; when the device
        gives up on some cells the whole lock-step is cut again on the host (gc_iteration: only those cells)."""
        r0 = runners[0]
        assert all(r.world == 1 and r.device_graph for r in runners)
        for k, (li, _) in enumerate(r0.sets):
            lk = r0._joint_set(runners, k)
            for kind, m in r0._proposals(li, iteration) if lk.n else ():
                t0 = time.perf_counter()
                for r, sh, base in lk.views:
                    r._propose(sh, kind, m)
                    r._graph(sh, lk.payload.data_ptr() + 20 * base)
                _, t1, t2 = r0._cut(lk, nthreads, partial=False)
                for r, sh, base in lk.views:
                    r._apply(sh, lk.masks.data_ptr() + base)
                r0._book(li, t0, t1, t2)
            for r in runners:
                r._log_set(k)
        r0._sync()

    def run(self, pm_iterations, iterations=0, graph_cut=None):
        """FastGCStereo::run for one view (LES/FastGCStereo.h:133-199): init, pmInit winner-take-all iterations, then
        `iterations` graph-cut iterations (their counter restarts at 0)."""
        self.init_labels()
        for it in range(pm_iterations):
            self.iteration(it)
        if iterations > 0:
            self.begin_gc(graph_cut)
            for it in range(iterations):
                self.gc_iteration(it)
            self.sync_gc_state()
        return self.labels, self.cur

    def disparities(self):
        return disparities(self.labels)

    def close(self):
        for lk in self._joint.values():
            if lk.batch is not None:
                lk.batch.destroy()
        for sh in [s for _, s in self.sets] + [self.init]:
            sh.batch.destroy()
            if sh.xchg is not None:
                sh.xchg.destroy()
