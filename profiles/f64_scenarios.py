#!/usr/bin/env python3
"""Writes the measured maxima of the fp64 free-running check of the landmark scenario kernel (fg64_rollout_scenario) as the second
half of profiles/f64_scenarios.md.  Run on an MI355X from the repository root:
    python profiles/f64_scenarios.py > measured.md
Every number is a max abs deviation over every env and agent (shared rewards: relative to max(1, |shared|)) of the whole
horizon run through the kernel's K-loop in ONE launch; the bound it is held to by tests/test_gpu_f64_scenarios.py stands beside it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]
from tests import scenario_cases as SC                     # noqa: E402
from tests import test_gpu_f64_scenarios as T              # noqa: E402
from tests.conftest import load_golden                     # noqa: E402

KEYS = ("pos", "vel", "opos", "ovel", "obs", "indiv", "shared")
cell = lambda e, k: "%.1e" % e[k] if k in e else "-"

print("## Measured maxima on an MI355X (fp64 build, free-running, one launch of the K-loop)\n")
print("pos / vel / opos / ovel: the state at the end of the launch (every step's velocities, and relative or absolute positions, are part of `obs`); obs / indiv / shared / done: every step.  `-`: not recorded by the fixture, or no obstacles.\n")
print("### The reference's landmark fixtures: bound %.0e\n" % T.FIXTURE_TOL)
print("| fixture | kind | N | envs x steps | " + " | ".join(KEYS) + " | done mismatches |")
print("|---|---|---|---|" + "---|" * len(KEYS) + "---|")
worst = {}
for name, kind in SC.FIXTURES:
    c = SC.fixture_case(name, load_golden(name))
    env = T._env(c, 0)
    out = env.rollout(c["acts"])
    e = T.fixture_errors(c, out, env.state())
    steps, B, N = c["acts"].shape[:3]
    bad = "-" if c["ref"]["done"] is None else "%d" % int((out["done"] != c["ref"]["done"]).sum())
    print("| %s | %s | %d | %d x %d | " % (name, kind, N, B, steps) + " | ".join(cell(e, k) for k in KEYS) + " | %s |" % bad)
    for k, v in e.items():
        worst[k] = max(worst.get(k, 0.0), v)
print("| **max** | | | | " + " | ".join(cell(worst, k) for k in KEYS) + " | |")

print("\n### Seeded oracle cases and the obstacle-floor cases, %d steps: bound %.0e\n" % (SC.SEEDED_STEPS, T.ORACLE_TOL))
print("| case | lanes per env x threads | staged image fits | " + " | ".join(KEYS) + " | (env, step) entries compared |")
print("|---|---|---|" + "---|" * len(KEYS) + "---|")
worst = {}
cases = [SC.seeded_case(i) for i in range(len(SC.SEEDED))] + [SC.floor_case(N, B) for N, B in SC.FLOOR_SHAPES]
for c in cases:
    r = SC.oracle_free_run(c["kind"], c["state"], c["acts"], c["P"], c["opts"])
    env = T._env(c, 0)
    out = env.rollout(c["acts"])
    e, share = T.oracle_errors(c, r, out, env.state())
    N = c["state"]["pos"].shape[1]
    G, threads, E, D = SC.geometry(c["kind"], N, c["P"])
    fits = SC.lds_bytes(c["kind"], N, c["P"], True) <= SC.FG64_LDS_LIMIT
    print("| %s | %d x %d | %s | " % (c["name"], G, threads, "yes" if fits else "no") + " | ".join(cell(e, k) for k in KEYS) + " | %.0f %% |" % (100 * share))
    for k, v in e.items():
        worst[k] = max(worst.get(k, 0.0), v)
print("| **max** | | | " + " | ".join(cell(worst, k) for k in KEYS) + " | |")
