"""The four calls over the resident scan at a pose — vgicp_evaluate_resident, vgicp_points_resident,
vgicp_align_resident_batch and vgicp_map_insert_resident_gated — walked down the ladder they share, on live contexts:
a fresh context (no map), a map but no scan, both, a scan whose preparation is still pending (settled, not refused), and
a context of several devices.  Every rung holds the status, the WHOLE text of vgicp_last_error and, on a refusal, that
every output keeps its 0xA5 fill (the two refusals the headers say write something: points' rule 10 and the gate's
rule 7, which leave the scan's size).  A successful call reports stats.seconds >= stats.device_seconds > 0 and the
launch count it always had.  The texts are literals: what these entries said before their host code shared one frame
(eskf_lio_amd/csrc/vgicp_capi_resident.inl, vgicp_resident_plan.h).  Nothing here provokes a fault: every rung is a
refusal on the host or a normal call.  The scene is tests/test_points.py's."""
import ctypes as C

import numpy as np
import pytest

import robust_reference as rr
from points_reference import QS
from test_align_batch import jitter_guesses, load_map

pytestmark = pytest.mark.gpu

NO_MAP = "no voxel map: call vgicp_map_reset first"
NO_SCAN = "no scan resident: call vgicp_scan_upload first"
SHARD = (" is not available on multi-device contexts, communicators and peer-connected contexts: "
         "the resident scan of a device is a shard there")
GATE_SHARD = "gated insertion works on a single-device context: the resident scan of a device is a shard here"
DP, U8P = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
K_EVAL, K_BATCH = 16, 4


@pytest.fixture(scope="module")
def scene():
    return rr.make_scene()


def filled(obj):
    C.memset(C.byref(obj), 0xA5, C.sizeof(obj))
    return obj


class Calls:
    """The four entries through the bare C ABI, every output filled with 0xA5 before the call."""

    def __init__(self, capi, scene):
        _, pts, _, T_true, _ = scene
        self.capi, self.lib, self.n = capi, capi.load_library(), len(pts)
        self.pose = capi.pose_to_abi(T_true)
        self.poses = np.ascontiguousarray(np.stack([capi.pose_to_abi(g) for g in jitter_guesses(K_EVAL)]))
        self.params = capi.Params(10, 0, 1e-6, 2.0, 0, 0)
        self.q = np.ascontiguousarray(QS, dtype=np.float64)
        # evaluate
        self.ev_out, self.ev_stats = (capi.Evaluation * K_EVAL)(), capi.EvalStats()
        # points
        self.planes = [np.empty(self.n) for _ in range(3)]
        self.status = np.empty(self.n, dtype=np.uint8)
        self.summary, self.pt_stats = capi.PointSummary(), capi.PointStats()
        # batch: of the per-hypothesis arrays only `status` is given (without it a degenerate hypothesis is the call's status)
        self.b_out, self.b_stats = np.empty((K_BATCH, 16)), capi.BatchStats()
        self.b_status = np.empty(K_BATCH, dtype=np.int32)
        # gated
        self.kept, self.g_stats = np.empty(self.n, dtype=np.uint8), capi.GatedInsertStats()
        self.before = {}

    def handle(self, ctx):
        return ctx._h if ctx is not None else None

    def evaluate(self, ctx, k=K_EVAL, poses="mine", out=True):
        C.memset(self.ev_out, 0xA5, C.sizeof(self.ev_out))
        filled(self.ev_stats)
        poses = self.poses if isinstance(poses, str) else poses
        return self.lib.vgicp_evaluate_resident(self.handle(ctx), k, poses.ctypes.data_as(DP) if poses is not None else None,
                                                self.ev_out if out else None, C.byref(self.ev_stats))

    def evaluate_untouched(self):
        return bytes(self.ev_out) == b"\xa5" * C.sizeof(self.ev_out) and bytes(self.ev_stats) == b"\xa5" * C.sizeof(self.ev_stats)

    def points(self, ctx, capacity=None, nq=len(QS)):
        for x in self.planes:
            x.view(np.uint8)[:] = 0xA5
        self.status[:] = 0xA5
        filled(self.summary), filled(self.pt_stats)
        d2, sq, w = (x.ctypes.data_as(DP) for x in self.planes)
        return self.lib.vgicp_points_resident(self.handle(ctx), self.pose.ctypes.data_as(DP),
                                              self.n if capacity is None else capacity, d2, sq, w,
                                              self.status.ctypes.data_as(U8P), nq, self.q.ctypes.data_as(DP),
                                              C.byref(self.summary), C.byref(self.pt_stats))

    def points_arrays_untouched(self):
        return all(np.all(x.view(np.uint8) == 0xA5) for x in self.planes) and np.all(self.status == 0xA5) and \
            bytes(self.pt_stats) == b"\xa5" * C.sizeof(self.pt_stats)

    def points_untouched(self):
        return self.points_arrays_untouched() and bytes(self.summary) == b"\xa5" * C.sizeof(self.summary)

    def batch(self, ctx, k=K_BATCH, guesses=True, out=True, params="mine"):
        self.b_out.view(np.uint8)[:] = 0xA5
        self.b_status.view(np.uint8)[:] = 0xA5
        filled(self.b_stats)
        self.b_stats.status = self.b_status.ctypes.data_as(C.POINTER(C.c_int32))
        self.b_stats.iterations = self.b_stats.converged = None
        self.b_stats.corr_count = None
        self.b_stats.normal_eq = None
        self.before["batch"] = bytes(self.b_stats)
        params = self.params if isinstance(params, str) else params
        return self.lib.vgicp_align_resident_batch(self.handle(ctx), k, self.poses.ctypes.data_as(DP) if guesses else None,
                                                   C.byref(params) if params is not None else None,
                                                   self.b_out.ctypes.data_as(DP) if out else None, C.byref(self.b_stats))

    def batch_untouched(self):
        return np.all(self.b_out.view(np.uint8) == 0xA5) and np.all(self.b_status.view(np.uint8) == 0xA5) and \
            bytes(self.b_stats) == self.before["batch"]

    def gated(self, ctx, capacity=None, gate=0.04):
        self.kept[:] = 0xA5
        filled(self.g_stats)
        return self.lib.vgicp_map_insert_resident_gated(self.handle(ctx), self.pose.ctypes.data_as(DP), 20, gate,
                                                        self.n if capacity is None else capacity,
                                                        self.kept.ctypes.data_as(U8P), C.byref(self.g_stats))

    def gated_untouched(self):
        return np.all(self.kept == 0xA5) and bytes(self.g_stats) == b"\xa5" * C.sizeof(self.g_stats)

    def entries(self):
        return (("evaluate", self.evaluate, self.evaluate_untouched), ("points", self.points, self.points_untouched),
                ("batch", self.batch, self.batch_untouched), ("gated", self.gated, self.gated_untouched))


def timed(stats):
    return stats.seconds >= stats.device_seconds > 0.0


def test_the_ladder_on_one_device(scene):
    from eskf_lio_amd import capi, synth
    vmap, pts, covs, _, _ = scene
    c = Calls(capi, scene)
    n = c.n
    ERR_ARG, NOT_READY, OK = capi.ERR_BAD_ARGUMENT, capi.ERR_NOT_READY, capi.OK

    def refused(ctx, name, rc, status, text, untouched):
        assert rc == status and ctx.last_error() == text, (name, rc, ctx.last_error())
        assert untouched(), name

    with capi.Context(0) as ctx:
        # ---- a fresh context.  What each entry asks of its arguments comes before what it asks of the context ----
        bad = c.poses.copy()
        bad[1, 13] = np.inf
        bad[3, 2] = np.nan
        for kwargs, text in ((dict(k=0), "k must be 1 .. VGICP_EVAL_MAX"), (dict(k=65), "k must be 1 .. VGICP_EVAL_MAX"),
                             (dict(poses=None), "NULL pointer"), (dict(out=False), "NULL pointer"),
                             (dict(poses=bad), "pose 1 has an entry that is not finite"),
                             (dict(k=1, poses=bad), NO_MAP)):           # only the first k poses are looked at
            refused(ctx, "evaluate", c.evaluate(ctx, **kwargs), NOT_READY if text == NO_MAP else ERR_ARG, text, c.evaluate_untouched)
        for kwargs, text in ((dict(k=0), "k must be 1 .. VGICP_BATCH_MAX"), (dict(k=65), "k must be 1 .. VGICP_BATCH_MAX"),
                             (dict(guesses=False), "NULL pose pointer"), (dict(out=False), "NULL pose pointer"),
                             (dict(params=None), "params is NULL"),
                             (dict(params=capi.Params(-1, 0, 1e-6, 2.0, 0, 0)), "max_iteration < 0")):
            refused(ctx, "batch", c.batch(ctx, **kwargs), ERR_ARG, text, c.batch_untouched)
        for name, call, untouched in c.entries():
            refused(ctx, name, call(ctx), NOT_READY, NO_MAP, untouched)
        # ---- a map, no scan ----
        load_map(ctx, vmap)
        for name, call, untouched in c.entries():
            refused(ctx, name, call(ctx), NOT_READY, NO_SCAN, untouched)
        # ---- both ----
        ctx.scan_upload(pts, covs)
        # the two refusals that know the scan's size only after settling, and leave it behind
        assert c.points(ctx, capacity=n - 1) == ERR_ARG and ctx.last_error() == "capacity smaller than the resident scan"
        assert c.points_arrays_untouched() and c.summary.points == n
        assert bytes(c.summary)[8:] == b"\xa5" * (C.sizeof(c.summary) - 8)
        assert c.gated(ctx, capacity=n - 1) == ERR_ARG and ctx.last_error() == "kept holds fewer than the scan's points"
        assert np.all(c.kept == 0xA5) and c.g_stats.points == n
        assert bytes(c.g_stats)[8:] == b"\xa5" * (C.sizeof(c.g_stats) - 8)
        ctx.frame_stats(reset=True)
        assert c.evaluate(ctx) == OK
        # 14 rows per pose (448 points each) of a budget of 4096: all of VGICP_EVAL_MAX would fit one launch pair
        assert (c.ev_stats.launches, c.ev_stats.poses_per_launch) == (2, 64) and timed(c.ev_stats)
        assert all(e.points == n and e.correspondences > 0 for e in c.ev_out)
        assert ctx.frame_stats().host_syncs == 1
        assert c.points(ctx) == OK
        assert c.pt_stats.launches == 2 + 1 + 3 and timed(c.pt_stats)      # 6000 pairs: the tile sort and three merges
        assert (c.summary.points, c.summary.matched) == (n, 5856) and np.all(c.status <= 1)
        assert ctx.frame_stats().host_syncs == 2
        assert c.batch(ctx) == OK
        print(f"batch: {c.b_stats.launches} launches, {c.b_stats.hypotheses_per_launch} hypotheses per launch")
        assert (c.b_stats.launches, c.b_stats.hypotheses_per_launch) == (1, K_BATCH) and timed(c.b_stats)
        assert np.all(np.isfinite(c.b_out)) and not c.b_status.any() and ctx.frame_stats().host_syncs == 3
        voxels = ctx.map_size()[0]
        ctx.frame_stats(reset=True)
        assert c.gated(ctx) == OK
        print(f"gated: {c.g_stats.launches} launches, {c.g_stats.refused} refused, {c.g_stats.new_voxels} new voxels")
        assert c.g_stats.launches == 1 + 1 + 4 + 1 and timed(c.g_stats)    # decide, prepare, the sort's four, apply
        assert (c.g_stats.points, c.g_stats.matched) == (n, 5856) and 0 < c.g_stats.refused < 5856
        assert int(np.count_nonzero(c.kept == 0)) == c.g_stats.refused and np.all(c.kept <= 1)
        assert ctx.frame_stats().host_syncs == 1 and ctx.map_size()[0] == voxels + c.g_stats.new_voxels
        # ---- a preparation that is still pending is settled by each of the four, not refused ----
        raw = synth.make_lidar_scan(3_000, seed=3)
        kept = ctx.scan_prepare(raw, None, None, None, 0.3, 30)[0]
        assert 0 < kept < 3_000
        for name, call, _ in c.entries():
            ctx.scan_prepare_async(raw, None, None, None, 0.3, 30)
            assert call(ctx) == OK, (name, ctx.last_error())
            assert ctx.scan_info()[0] == kept
            size = {"evaluate": c.ev_out[0].points, "points": c.summary.points, "batch": kept, "gated": c.g_stats.points}[name]
            assert size == kept, name
            assert timed({"evaluate": c.ev_stats, "points": c.pt_stats, "batch": c.b_stats, "gated": c.g_stats}[name]), name


def test_several_devices(scene):
    """Context([0, 0]): two sub-contexts on the one device.  Evaluate and the report refuse it for what it is, before
    they ask for a map; the gated insertion asks its insertion's questions first (no map, no scan) and refuses it then;
    the batch does not refuse it at all: it runs as k aligns of the group."""
    from eskf_lio_amd import capi
    vmap, pts, covs, _, _ = scene
    c = Calls(capi, scene)
    with capi.Context([0, 0]) as multi:
        for loaded in (False, True):
            if loaded:
                load_map(multi, vmap)
                multi.scan_upload(pts, covs)
            assert c.evaluate(multi) == capi.ERR_BAD_ARGUMENT and multi.last_error() == "vgicp_evaluate_resident" + SHARD
            assert c.evaluate_untouched()
            assert c.points(multi) == capi.ERR_BAD_ARGUMENT and multi.last_error() == "vgicp_points_resident" + SHARD
            assert c.points_untouched()
            if not loaded:
                assert c.gated(multi) == capi.ERR_NOT_READY and multi.last_error() == NO_MAP and c.gated_untouched()
        bad = c.poses.copy()
        bad[2, 0] = np.nan
        assert c.evaluate(multi, poses=bad) == capi.ERR_BAD_ARGUMENT                   # the poses before the context
        assert multi.last_error() == "pose 2 has an entry that is not finite" and c.evaluate_untouched()
        assert c.gated(multi) == capi.ERR_BAD_ARGUMENT and multi.last_error() == GATE_SHARD and c.gated_untouched()
        assert c.gated(multi, capacity=0) == capi.ERR_BAD_ARGUMENT and multi.last_error() == GATE_SHARD
        assert c.batch(multi, k=2) == capi.OK, multi.last_error()
        assert c.b_stats.hypotheses_per_launch == 1 and c.b_stats.launches >= 2 and timed(c.b_stats)
        assert np.all(np.isfinite(c.b_out[:2])) and np.all(c.b_out[2:].view(np.uint8) == 0xA5)
