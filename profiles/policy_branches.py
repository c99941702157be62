"""The numbers of profiles/policy_branches.md that need no GPU: the branch census of the controller's earlier inputs and of the
designed cases (tests/policy_testlib.py), the rows each mutant of the fp64 model moves on either, and the near-tie rows of the
two largest random cases of tests/test_gpu_policy.py.    python profiles/policy_branches.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-formation_amd")):
    sys.path.insert(0, p)

from oracle import formation_oracle as O                    # noqa: E402
from tests import policy_testlib as T                       # noqa: E402
from tests import test_policy_cases_cpu as C                # noqa: E402
from tests.conftest import load_golden                      # noqa: E402


def main():
    print("== earlier inputs: census, and rows (of how many) each mutant moves by more than the bound / ten times the bound")
    total, moved, rows = {}, {m: [0, 0] for m in T.MUTANTS}, 0
    for name, per, obs in C.earlier_inputs(load_golden):
        c, _ = C.census(obs, per)
        for k, v in c.items():
            k = k.split("@")[0]
            total[k] = total.get(k, 0) + v
        base = T.model(obs, per)
        rows += base.shape[0] * base.shape[1]
        for m in T.MUTANTS:
            err = np.abs(T.model(obs, per, m) - base).max(-1) / T.bound(base)[:, None]
            moved[m][0] += int((err > 1).sum())
            moved[m][1] += int((err > 10).sum())
    print(total)
    for m in T.MUTANTS:
        print("  %-24s %6d %6d of %d" % (m, moved[m][0], moved[m][1], rows))
    print("== designed cases: census per hierarchy (all classes), rows moved per mutant and class")
    for per, L in T.HIERARCHIES:
        case, obs, sl = T.stacked(per, L)
        c, _ = C.census(obs, per)
        print("(%d,%d) N=%d envs=%d" % (per, L, per ** L, len(obs)), {k: v for k, v in c.items() if v})
        for m, by in C.moved_rows(per, L).items():
            print("    %-24s %s" % (m, "  ".join("%s %d" % kv for kv in by.items() if kv[1])))
    print("== near-tie rows (margin < 1e-6) of the two largest random cases of tests/test_gpu_policy.py, first two envs")
    for N, per, B in ((729, 3, 2), (1024, 2, 2)):
        st = O.reset_hd(7 + 1000 * np.arange(B), N)
        f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
        obs = f32(O.observation_hd(f32(st["pos"] * 0.5), st["vel"], f32(st["ideal_shape"]), f32(st["ideal_vel"])))
        mg = np.stack([O.bfs_margins(list(obs[b]), per) for b in range(2)])
        print("  N=%d per=%d: %d of %d rows, smallest margin %.3g" % (N, per, int((mg < 1e-6).sum()), mg.size, mg.min()))


if __name__ == "__main__":
    main()
