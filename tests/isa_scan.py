"""What a built HIP shared library's gfx950 code object holds, read without a GPU.  The one place that unbundles it.

`kernel_resources(path)` -> [{name, demangled, private_segment, vgpr, sgpr, vgpr_spill, sgpr_spill, kernarg}, ...] from the code
    object's metadata notes.  Used by tests/test_build_resources.py (every shipped kernel runs without scratch memory).
`kernarg_sizes(path)` -> {mangled name: .kernarg_segment_size}.
`kernel_disassembly(path)` -> {mangled name: [instruction, ...]} with comments, addresses and label operands removed, so that
    two builds of the same source compare equal although their files differ bytewise.

As a command:
    python3 tests/isa_scan.py [lib.so]              every kernel that has a private segment or spills
    python3 tests/isa_scan.py --diff OLD.so NEW.so  the kernels added, removed and changed between two builds; exit status 1
                                                    if a kernel present in both differs (the check of a refactor that must
                                                    leave every kernel's instructions alone)"""
import contextlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_BIN = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def _llvm(tool, *args, **kw):
    return subprocess.run([os.path.join(LLVM_BIN, tool)] + list(args), check=True, **kw)


@contextlib.contextmanager
def code_objects(lib_path, arch="gfx950"):
    """The paths of the `arch` code objects embedded in `lib_path`, unbundled into a directory that lives as long as the
    `with` block."""
    tmp = tempfile.mkdtemp(prefix="fg_isa_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib_path, local)
        # llvm-objdump --offloading writes every bundle entry next to its input: <input>.<n>.<triple>
        _llvm("llvm-objdump", "--offloading", local, cwd=tmp, stdout=subprocess.DEVNULL)
        objs = sorted(os.path.join(tmp, f) for f in os.listdir(tmp) if f.endswith(arch))
        if not objs:
            raise RuntimeError("no %s code object in %s" % (arch, lib_path))
        yield objs
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def demangle(names):
    filt = shutil.which("c++filt") or os.path.join(LLVM_BIN, "llvm-cxxfilt")
    try:
        return subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        return list(names)


def kernel_resources(lib_path, arch="gfx950"):
    out = []
    with code_objects(lib_path, arch) as objs:
        for obj in objs:
            notes = _llvm("llvm-readelf", "--notes", obj, capture_output=True, text=True).stdout
            for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                def field(key, default=0):
                    m = re.search(r"\.%s:\s+(\d+)" % key, block)
                    return int(m.group(1)) if m else default
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                out.append({"name": name, "private_segment": field("private_segment_fixed_size"), "vgpr": field("vgpr_count"),
                            "sgpr": field("sgpr_count"), "vgpr_spill": field("vgpr_spill_count"),
                            "sgpr_spill": field("sgpr_spill_count"), "kernarg": field("kernarg_segment_size")})
    for k, d in zip(out, demangle([k["name"] for k in out])):
        k["demangled"] = d
    return out


def kernarg_sizes(lib_path, arch="gfx950"):
    """.kernarg_segment_size of every kernel in the code object, by mangled name."""
    return {k["name"]: k["kernarg"] for k in kernel_resources(lib_path, arch)}


def kernel_disassembly(lib_path, arch="gfx950"):
    """{mangled kernel name: its instruction lines}.  A line is mnemonic and operands: comments, the `<label>` operands and the
    target addresses of branches are stripped, as is the padding between kernels (objdump's `...` and the `s_nop` lines behind a
    kernel's last `s_endpgm`), so code that only moved compares equal."""
    names = {k["name"] for k in kernel_resources(lib_path, arch)}
    out, cur = {}, None
    with code_objects(lib_path, arch) as objs:
        for obj in objs:
            text = _llvm("llvm-objdump", "-d", "--no-show-raw-insn", obj, capture_output=True, text=True).stdout
            for line in text.split("\n"):
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), []) if m.group(1) in names else None
                elif cur is not None and line.strip():
                    ins = re.sub(r"<[^>]*>", "", re.sub(r"\s*//.*$", "", line)).strip()
                    if re.match(r"s_(c?branch|call)", ins):
                        ins = ins.split()[0]
                    if ins and ins != "...":               # "...": zero padding between kernels, elided by objdump
                        cur.append(ins)
    for code in out.values():                              # the s_nop lines that align whatever follows the kernel's end
        if "s_endpgm" in code:
            end = len(code) - code[::-1].index("s_endpgm")
            if all(ins.startswith("s_nop") for ins in code[end:]):
                del code[end:]
    return out


def diff_libraries(old, new, arch="gfx950"):
    """(added, removed, changed, same): sorted mangled kernel names."""
    a, b = kernel_disassembly(old, arch), kernel_disassembly(new, arch)
    both = set(a) & set(b)
    changed = sorted(k for k in both if a[k] != b[k])
    return sorted(set(b) - set(a)), sorted(set(a) - set(b)), changed, sorted(both - set(changed))


def _diff_main(old, new):
    added, removed, changed, same = diff_libraries(old, new)
    for title, names in (("added", added), ("removed", removed), ("changed", changed)):
        for name, dem in zip(names, demangle(names)):
            print("%-8s%s" % (title, dem[:150]))
    print("%s -> %s: %d kernels in both, %d identical, %d changed, %d added, %d removed"
          % (old, new, len(same) + len(changed), len(same), len(changed), len(added), len(removed)))
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--diff":
        if len(sys.argv) != 4:
            sys.exit("usage: isa_scan.py --diff OLD.so NEW.so")
        sys.exit(_diff_main(sys.argv[2], sys.argv[3]))
    here = os.path.dirname(os.path.abspath(__file__))
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "gym-formation_amd", "lib", "libformation_hip.so")
    ks = kernel_resources(lib)
    bad = [k for k in ks if k["private_segment"] or k["vgpr_spill"]]
    for k in sorted(bad, key=lambda k: k["demangled"]):
        print("private %4d B  vgpr %3d  vgpr spills %3d  sgpr spills %3d  %s"
              % (k["private_segment"], k["vgpr"], k["vgpr_spill"], k["sgpr_spill"], k["demangled"][:130]))
    spilled = [k for k in ks if k["sgpr_spill"] and not (k["private_segment"] or k["vgpr_spill"])]
    print("%d kernels, %d with a private segment or VGPR spills, %d more with SGPR spills (to VGPR lanes) only"
          % (len(ks), len(bad), len(spilled)))
    for k in sorted(spilled, key=lambda k: -k["sgpr_spill"])[:40]:
        print("   sgpr spills %3d  vgpr %3d  %s" % (k["sgpr_spill"], k["vgpr"], k["demangled"][:130]))
