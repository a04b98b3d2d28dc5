"""Every instantiation of a round kernel that a single-device context can reach (eskf_lio_amd/csrc/vgicp_launch_plan.h:
kIterateVariants, kCloseVariants, kPersistentVariants without the multi-rank ones) is launched, and computes what the other
path computes.  The lists, the table of kernel pointers and the LDS limits are one set by construction; this is the guard
that the set still reaches the device: a persistent launch with 150 KB of dynamic LDS fails when its instantiation's limit
was not raised, and a dropped flag shows as another instantiation's result.

The map is conftest's c1_inputs; the robust mode and the prior are tests/test_robust.py's PAIR and tests/test_prior.py's
dense prior; path against path within the tolerances those tests use for the same comparison (rtol 1e-11, atol 1e-7)."""
import numpy as np
import pytest

from test_align_batch import assert_same_bits, load_map
from test_prior import PRIORS, offset_pose
from test_robust import PAIR

pytestmark = pytest.mark.gpu

COUNTER_FALLBACKS = 1
SETTINGS = ("plain", "robust", "prior", "both")
ROUNDS, TSQ, COS = 4, 1e-12, 2.0          # every round runs: no align converges
RTOL, ATOL = 1e-11, 1e-7


def make_ctx(monkeypatch, vmap, **env):
    """A context created under these variables (all of them are read when a context is created), with the map loaded."""
    from eskf_lio_amd import capi
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    ctx = capi.Context(0)
    for name in env:
        monkeypatch.delenv(name)
    load_map(ctx, vmap)
    return ctx


def apply(ctx, setting, guess):
    if setting in ("robust", "both"):
        ctx.set_robust(*PAIR)
    else:
        ctx.set_robust("none", 1.0, 0.0)
    if setting in ("prior", "both"):
        ctx.set_pose_prior(offset_pose(guess, 0.03, 0.5, seed=22), PRIORS["dense"])
    else:
        ctx.clear_pose_prior()


def persistent_checked(ctx, guess, what):
    """One persistent align of the resident scan, held against the per-launch loop and against a second run."""
    from eskf_lio_amd import capi
    one = ctx.align_resident(guess, ROUNDS, TSQ, COS, allow_degenerate=True)
    loop = ctx.align_resident(guess, ROUNDS, TSQ, COS, flags=capi.FLAG_NO_PERSISTENT, allow_degenerate=True)
    again = ctx.align_resident(guess, ROUNDS, TSQ, COS, allow_degenerate=True)
    assert one.launches == 1 and ctx.counter(COUNTER_FALLBACKS) == 0, what
    assert loop.launches > 1 and one.iterations == loop.iterations == ROUNDS, what
    assert np.array_equal(one.corr_count, loop.corr_count), what
    worst = np.abs(one.normal_eq - loop.normal_eq).max()
    print(f"{what}: counts {one.corr_count[:ROUNDS]}, persistent against loop: largest normal_eq difference {worst:.3e}")
    assert np.allclose(one.normal_eq, loop.normal_eq, rtol=RTOL, atol=ATOL), what
    assert_same_bits(again, one, what + ", second run")
    return one


@pytest.mark.parametrize("n", [700, 3000])
def test_every_single_device_persistent_variant(c1_inputs, monkeypatch, n):
    """Two workgroups (VGICP_PERSIST_GRID=2).  700 points: one point per thread, with the prefetch area.  3 000 points:
    four per thread at most, so persistent_lds_plan gives 3 memos and a stash that fills the rest of 150 KB — the launch
    that needs the raised LDS limit.  Plain, Cauchy with a gate, a pose prior, both; and the plain launch of a context
    with VGICP_DEBUG_STAMPS=1.  Each: one launch, no give-up, the loop's counts, the loop's normal equations within the
    tolerances, the same bits twice.  Across them, what a dropped flag cannot hide: the robust result differs from the
    plain one with fewer correspondences in the first round, the prior's differs, the stamps launch returns the plain
    launch's bits."""
    from eskf_lio_amd import synth
    vmap, pts, covs = c1_inputs
    guess = synth.default_guess()
    got = {}
    with make_ctx(monkeypatch, vmap, VGICP_PERSIST_GRID="2") as ctx:
        ctx.scan_upload(pts[:n], covs[:n])
        for setting in SETTINGS:
            apply(ctx, setting, guess)
            got[setting] = persistent_checked(ctx, guess, f"n {n} {setting}")
    with make_ctx(monkeypatch, vmap, VGICP_PERSIST_GRID="2", VGICP_DEBUG_STAMPS="1") as ctx:
        ctx.scan_upload(pts[:n], covs[:n])
        stamps = persistent_checked(ctx, guess, f"n {n} stamps")
    assert_same_bits(stamps, got["plain"], f"n {n}: stamps against plain")
    plain = got["plain"]
    for setting in ("robust", "both"):
        assert not np.array_equal(got[setting].normal_eq, plain.normal_eq), setting
        assert got[setting].corr_count[0] < plain.corr_count[0], (setting, got[setting].corr_count, plain.corr_count)
    assert not np.array_equal(got["prior"].pose, plain.pose) and not np.array_equal(got["prior"].normal_eq, plain.normal_eq)
    assert not np.array_equal(got["both"].pose, got["robust"].pose)


def test_every_block_size_of_the_per_launch_loop(c1_inputs, monkeypatch):
    """VGICP_ITER_BLOCK in {256, 512, 1024} x the four settings on 700 points under FLAG_NO_PERSISTENT: every
    iterate_kernel and close_kernel instantiation.  More than one launch, the same counts at every block size, normal
    equations within the tolerances (the partition of the points into workgroups differs with the block size)."""
    from eskf_lio_amd import capi, synth
    vmap, pts, covs = c1_inputs
    guess = synth.default_guess()
    got = {}
    for block in (256, 512, 1024):
        with make_ctx(monkeypatch, vmap, VGICP_ITER_BLOCK=str(block)) as ctx:
            ctx.scan_upload(pts[:700], covs[:700])
            for setting in SETTINGS:
                apply(ctx, setting, guess)
                r = ctx.align_resident(guess, ROUNDS, TSQ, COS, flags=capi.FLAG_NO_PERSISTENT, allow_degenerate=True)
                assert r.launches > 1 and r.iterations == ROUNDS, (block, setting)
                got[block, setting] = r
    for setting in SETTINGS:
        ref = got[512, setting]
        for block in (256, 1024):
            r = got[block, setting]
            worst = np.abs(r.normal_eq - ref.normal_eq).max()
            print(f"{setting}, block {block} against 512: largest normal_eq difference {worst:.3e}")
            assert np.array_equal(r.corr_count, ref.corr_count), (block, setting)
            assert np.allclose(r.normal_eq, ref.normal_eq, rtol=RTOL, atol=ATOL), (block, setting)
