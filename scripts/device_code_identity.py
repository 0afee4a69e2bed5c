#!/usr/bin/env python3
"""Proof that a refactor left a source's device code alone: python scripts/device_code_identity.py SRC.hip OLD_TREE NEW_TREE

Compiles pixie_amd/csrc/SRC.hip of both trees device-only with the flags of NEW_TREE's pixie_amd/build.py (FLAGS + EXTRA_FLAGS),
once plain and once with -DPIXIE_DIAG, and compares the gfx950 code objects section by section: .text (the instructions),
.rodata (the kernel descriptors), the notes (kernel metadata: registers, LDS, kernarg layout) and the list of kernel symbols.
Whole files are not compared: two compiles of one source already differ in the __hip_cuid_<hash> symbol.  One line per flavour;
exit status 1 when anything differs.  Needs hipcc only, no GPU."""
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile


def load_build(tree):
    spec = importlib.util.spec_from_file_location("_pixie_build", os.path.join(tree, "pixie_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def tool(hipcc, name):
    p = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", name)
    return p if os.path.exists(p) else name


def start_compile(b, tree, src, diag, out):
    cmd = [b._hipcc()] + b.FLAGS + b.EXTRA_FLAGS.get(src, []) + (["-DPIXIE_DIAG"] if diag else []) + \
          ["--cuda-device-only", "-c", os.path.join(tree, "pixie_amd", "csrc", src), "-o", out]
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def facts(b, co):
    """(.text bytes, .rodata bytes, notes text, sorted kernel names) of a device-only object."""
    hipcc = b._hipcc()
    elf = co + ".elf"
    subprocess.check_call([tool(hipcc, "clang-offload-bundler"), "--type=o", "--targets=hip-amdgcn-amd-amdhsa--" + b.ARCH,
                           "--input=" + co, "--output=" + elf, "--unbundle"])
    out = {}
    for sec in (".text", ".rodata"):
        raw = elf + sec
        subprocess.check_call([tool(hipcc, "llvm-objcopy"), "-O", "binary", "--only-section=" + sec, elf, raw])
        with open(raw, "rb") as f:
            out[sec] = f.read()
    out["notes"] = subprocess.check_output([tool(hipcc, "llvm-readelf"), "--notes", elf], text=True)
    syms = subprocess.check_output([tool(hipcc, "llvm-readelf"), "--symbols", "--wide", elf], text=True)
    out["kernels"] = "\n".join(sorted(w[-1] for w in (l.split() for l in syms.splitlines()) if len(w) >= 8 and w[3] == "FUNC" and w[6] != "UND"))
    return out


def main(argv):
    if len(argv) != 4:
        sys.exit(__doc__)
    src, old, new = argv[1], os.path.abspath(argv[2]), os.path.abspath(argv[3])
    b = load_build(new)
    same = True
    with tempfile.TemporaryDirectory() as tmp:
        jobs = {(t, d): os.path.join(tmp, f"{t}{int(d)}.co") for t in ("old", "new") for d in (False, True)}
        procs = {k: start_compile(b, old if k[0] == "old" else new, src, k[1], v) for k, v in jobs.items()}
        for k, p in procs.items():
            log, _ = p.communicate()
            if p.returncode != 0:
                sys.exit(f"hipcc failed on the {k[0]} tree{' -DPIXIE_DIAG' if k[1] else ''}:\n{log}")
        for diag in (False, True):
            fo, fn = facts(b, jobs[("old", diag)]), facts(b, jobs[("new", diag)])
            parts = []
            for key in (".text", ".rodata", "notes", "kernels"):
                eq = fo[key] == fn[key]
                same = same and eq
                data = fn[key] if isinstance(fn[key], bytes) else fn[key].encode()
                size = f"0x{len(data):x} bytes" if key != "kernels" else f"{len(fn[key].splitlines())} functions"
                parts.append(f"{key} {'identical' if eq else 'DIFFERENT'} ({size}, sha256 {hashlib.sha256(data).hexdigest()[:12]})")
            print(f"{src}{' -DPIXIE_DIAG' if diag else ''}: " + "; ".join(parts), flush=True)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
