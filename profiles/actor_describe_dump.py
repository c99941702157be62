"""Print what every describe twin of the formation_hd_env actor entries (fg_describe_actor*_launch) answers over a grid of
shapes and members, for the given build of libformation_hip.so: one line per call with the status and the describe string, or
fg_last_error()'s text where the call is refused.  Touches no device (the twins never do).

    python profiles/actor_describe_dump.py LIB.so > dump.txt

Two builds that dispatch alike print the same bytes: the kernel names, grids and LDS sizes of every reachable (family, member,
N, H), and the code and text of every refusal.  The grid: N in {3, 4, 5, 8, 9, 16, 25, 27, 32, 81}, hidden in {32, 48, 64, 128},
B in {1, 8, 4096}; with and without log_std; with and without the input norm; both 16-bit formats and an invalid one; both
action modes and both `greedy` values; the OU twins with and without in_bn."""
import ctypes
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gym-formation_amd"))
from formation_gym import _native as nat  # noqa: E402

NS, HS, BS, K = (3, 4, 5, 8, 9, 16, 25, 27, 32, 81), (32, 48, 64, 128), (1, 8, 4096), 20
ADDR = 4096                                            # a stand-in address: only NULL-ness and alignment are looked at
FORMATS = (nat.FG_OBS_F16, nat.FG_OBS_BF16, 7)
MODES = (nat.FG_ACT_ONEHOT5, nat.FG_ACT_INDEX)


def params():
    p = nat.FgParams()
    p.dt, p.damping, p.contact_force, p.contact_margin = 0.1, 0.25, 100.0, 0.001
    p.sensitivity, p.mass, p.dist_min, p.collide_thresh, p.world_length = 5.0, 1.0, 0.06, 0.03, 100
    return p


def calls(N, H):
    """(label, twin, its arguments between params and B) of every call made at one (N, H)."""
    def actors(tanh):
        return (nat.FgActor * N)(*[nat.FgActor(H, tanh, *[ADDR] * 6) for _ in range(N)])
    actor, logits = actors(1), actors(0)               # (the categorical head takes no tanh)
    norms = [nat.FgActorNorm(*[ADDR] * 6, 1e-5, 1e-5, 1e-5, in_norm) for in_norm in (0, 1)]
    gru = nat.FgActorGru(*[ADDR] * 6, 1e-5)
    bns = (nat.FgActorInBn * N)(*[nat.FgActorInBn(ADDR, ADDR, ADDR, ADDR, 1e-5) for _ in range(N)])
    ou = nat.FgActorOu(0.15, 0.0, 0.2, 0.3, 1.0)
    bodies = [("plain", None, None)]                   # the bodies that have categorical and 16-bit members
    bodies += [("norm in%d" % i, norms[i], None) for i in (0, 1)] + [("gru in%d" % i, norms[i], gru) for i in (0, 1)]
    yield "det", "fg_describe_actor_launch", (actor,)
    for ls in (None, ADDR):
        tag = "log_std %d" % (ls is not None)
        yield "sample " + tag, "fg_describe_actor_sample_launch", (actor, ls)
        yield "per_agent " + tag, "fg_describe_actor_per_agent_launch", (actor, ls)
        for i in (0, 1):
            yield "norm in%d %s" % (i, tag), "fg_describe_actor_norm_launch", (actor, norms[i], ls)
            yield "gru in%d %s" % (i, tag), "fg_describe_actor_gru_launch", (actor, norms[i], gru, ls)
        yield "bn " + tag, "fg_describe_actor_bn_launch", (actor, bns, ls)
        yield "bn_per_agent " + tag, "fg_describe_actor_bn_per_agent_launch", (actor, bns, ls)
        for (body, norm, g), fmt in itertools.product(bodies, FORMATS):
            yield "obs16 fmt %d %s %s" % (fmt, body, tag), "fg_describe_actor_obs16_launch", (fmt, actor, norm, g, ls)
    for bn in (None, bns):
        yield "ou in_bn %d" % (bn is not None), "fg_describe_actor_ou_launch", (actor, bn, ou)
        yield "ou_per_agent in_bn %d" % (bn is not None), "fg_describe_actor_ou_per_agent_launch", (actor, bn, ou)
    for (body, norm, g), mode, greedy in itertools.product(bodies, MODES, (0, 1)):
        tag = "%s mode %d greedy %d" % (body, mode, greedy)
        yield "cat " + tag, "fg_describe_actor_cat_launch", (logits, norm, g, mode, greedy)
        for fmt in FORMATS:
            yield "cat_obs16 fmt %d %s" % (fmt, tag), "fg_describe_actor_cat_obs16_launch", (fmt, logits, norm, g, mode, greedy)


def main(argv):
    lib = ctypes.CDLL(argv[1])
    for name, (res, args) in nat.SIGNATURES.items():
        if name == "fg_last_error" or name.startswith("fg_describe_actor"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    p, buf = params(), ctypes.create_string_buffer(512)
    for N, H in itertools.product(NS, HS):
        for label, twin, lead in calls(N, H):
            for B in BS:
                rc = getattr(lib, twin)(p, *lead, B, N, K, 1, buf, len(buf))
                text = buf.value.decode() if rc == nat.FG_OK else lib.fg_last_error().decode("utf-8", "replace")
                print("N %d H %d B %d %s: %d %s" % (N, H, B, label, rc, text))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
