"""Compare the per-kernel metadata (tests/isa_scan.kernel_resources: registers, LDS, scratch, spills, ...) of two builds of
libformation_hip.so, for the kernels whose demangled name contains one of the given substrings.

    python profiles/kernel_metadata_diff.py OLD.so NEW.so [substring ...]

Default substrings: the formation_hd_env actor kernels (six families, each deterministic and Gaussian, their OU members and the
three categorical members).  Prints one
line per substring - kernels compared, kernels that differ - then every differing kernel with both records, and exits 1 if any
differ or a kernel is missing on either side."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.isa_scan import kernel_resources  # noqa: E402

FAMILIES = ("actor_rollout_kernel<", "actor_sample_kernel<", "pa_actor_kernel<", "pa_sample_kernel<", "ln_actor_kernel<",
            "ln_sample_kernel<", "gru_actor_kernel<", "gru_sample_kernel<", "::bn_actor_kernel<", "::bn_sample_kernel<",
            "pa_bn_actor_kernel<", "pa_bn_sample_kernel<", "::ou_actor_kernel<", "::pa_ou_actor_kernel<", "::bn_ou_actor_kernel<",
            "pa_bn_ou_actor_kernel<", "::cat_actor_kernel<", "ln_cat_actor_kernel<", "gru_cat_actor_kernel<",
            "::actor_sample_obs16<", "::ln_sample_obs16<", "::gru_sample_obs16<", "::cat_actor_obs16<", "::ln_cat_actor_obs16<",
            "::gru_cat_actor_obs16<")


def main(argv):
    old, new = argv[1], argv[2]
    families = tuple(argv[3:]) or FAMILIES
    a = {k["demangled"]: k for k in kernel_resources(old)}
    b = {k["demangled"]: k for k in kernel_resources(new)}
    bad = 0
    for fam in families:
        names = sorted(set(n for n in a if fam in n) | set(n for n in b if fam in n))
        diff = [n for n in names if a.get(n) != b.get(n)]
        print("%-24s %3d kernels, %d differ" % (fam, len(names), len(diff)))
        for n in diff:
            print("  ", n, "\n     old", a.get(n), "\n     new", b.get(n))
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
