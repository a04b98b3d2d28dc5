"""Child process of tests/test_prepare_routes.py: the scan preparation's routes x deskew variants at the smallest shapes
that reach every branch, in an environment the parent chose (VGICP_STAGE_LIMIT is read once per process: unset, sweeps
that are not staged ahead are staged by the copy crew; 1, they go up in place).  Every variant is prepared through
scan_prepare_async + scan_info + scan_download and again through sweep_stage + scan_prepare_staged_async, and compared
with vgicp_deskew + vgicp_preprocess on a second context (their own kernels).  Prints one JSON line.
usage: python prepare_routes_worker.py [--dump FILE.npz]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eskf_lio_amd import capi, synth  # noqa: E402

SIZES = (3_000, 70_000)   # one copy unit; above the crew's 1 MB helper threshold (1.68 MB of points) and several units
VARIANTS = ("none", "ordered-8", "ordered-4100", "swapped-8")


def variant_states(name, n):
    """-> (states or None, capture times or None)"""
    if name == "none":
        return None, None
    count = 4100 if name == "ordered-4100" else 8
    st = synth.make_imu_states(count, seed=count)
    # the sweep spans states 1 .. count - 3: every state in between can own points
    t = synth.make_point_times(n, st[1, 0] + 1e-6, st[-3, 0] + 1e-6, seed=9)
    if name == "swapped-8":   # one swapped pair of timestamps among the states that own points: not ordered, the serial walk
        st[3, 0], st[4, 0] = st[4, 0], st[3, 0]
    return st, t


def prepared(ctx):
    kept, moved, _ = ctx.scan_info()
    pts, covs = ctx.scan_download()
    return kept, moved, pts.copy(), covs.copy()


def attempt(call):
    """-> (result, None) or (None, [code, text])"""
    try:
        return call(), None
    except capi.VgicpError as e:
        return None, [e.code, str(e)]


def main():
    dump = sys.argv[sys.argv.index("--dump") + 1] if "--dump" in sys.argv else None
    cases, arrays = [], {}
    with capi.Context(0) as a, capi.Context(0) as b:
        for n in SIZES:
            raw = synth.make_lidar_scan(n, seed=41, extent=30.0)
            for name in VARIANTS:
                st, t = variant_states(name, n)
                case = {"n": n, "variant": name}
                if st is None:
                    kp, kc, _ = b.preprocess(raw, 0.3, 30)
                    done = 0
                else:
                    dp, done = b.deskew(raw, t, st)
                    kp, kc, _ = b.preprocess(dp, 0.3, 30)
                case["want"] = [len(kp), done]
                a.frame_stats(reset=True)

                def direct():
                    a.scan_prepare_async(raw, t, st, None, 0.3, 30)
                    case["copies"] = int(a.frame_stats().copies)   # copy commands of the enqueue alone
                    return prepared(a)

                def ahead():
                    a.scan_prepare_staged_async(a.sweep_stage(raw, t), st, None, 0.3, 30)
                    return prepared(a)

                for route, call in (("direct", direct), ("ahead", ahead)):
                    got, err = attempt(call)
                    case[route + "_error"] = err
                    if got is not None:
                        kept, moved, gp, gc = got
                        case[route] = [kept, moved]
                        case[route + "_equal"] = bool(kept == len(kp) and moved == done and np.array_equal(gp, kp) and
                                                      np.array_equal(gc, kc))
                        arrays[f"{n}_{name}_{route}_pts"], arrays[f"{n}_{name}_{route}_cov"] = gp, gc
                        arrays[f"{n}_{name}_{route}_counts"] = np.array([kept, moved])
                print(json.dumps(case), file=sys.stderr, flush=True)
                cases.append(case)
    if dump:
        np.savez(dump, **arrays)
    print(json.dumps({"stage_limit": os.environ.get("VGICP_STAGE_LIMIT"), "cases": cases}), flush=True)


if __name__ == "__main__":
    main()
