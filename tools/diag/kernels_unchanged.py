"""Do two versions of one HIP source compile to the same kernels?  (needs no GPU)

    python tools/diag/kernels_unchanged.py OLD.hip NEW.hip

Both are compiled device-only with build.py's flags for NEW's file name.  Kernels are emitted in order of first use in host
code, so a host-only change moves them around: the code objects are compared kernel by kernel -- the bytes of every FUNC
symbol, and the kernel's entry of the metadata note (registers, LDS, scratch, kernarg layout) -- never as whole files.
Exit status 0: same symbol set, no differing body, same metadata."""
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile

import yaml

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(REPO, "self-paced-contrastive-learning_amd")
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")


def _build_py():
    spec = importlib.util.spec_from_file_location("spcl_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernels(src, flags_name, tmp, tag):
    """{symbol: (sha256 of its bytes, size)}, {kernel name: metadata entry} of src's gfx950 code object"""
    b = _build_py()
    co = os.path.join(tmp, tag + ".co")
    cmd = [b.HIPCC] + b._flags_for(flags_name) + ["-I", os.path.join(PKG, "csrc"), "-x", "hip", "--offload-device-only",
                                                  "--no-gpu-bundle-output", "-c", os.path.abspath(src), "-o", co]
    subprocess.run(cmd, check=True, cwd=os.path.join(PKG, "csrc"))
    blob = open(co, "rb").read()
    sections, funcs = {}, {}
    for ln in subprocess.run([READELF, "-S", "-W", co], check=True, capture_output=True, text=True).stdout.splitlines():
        f = ln.replace("[", " ").replace("]", " ").split()
        if len(f) >= 6 and f[0].isdigit() and f[0] != "0":
            sections[int(f[0])] = (int(f[3], 16), int(f[4], 16))  # address, file offset
    for ln in subprocess.run([READELF, "-s", "-W", co], check=True, capture_output=True, text=True).stdout.splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6].isdigit():
            addr, off = sections[int(f[6])]
            start = int(f[1], 16) - addr + off
            funcs[f[7]] = (hashlib.sha256(blob[start:start + int(f[2])]).hexdigest(), int(f[2]))
    notes = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, text=True).stdout
    doc = notes[notes.index("---"):notes.index("\n...") if "\n..." in notes else len(notes)]
    meta = {k[".name"]: k for k in yaml.safe_load(doc)["amdhsa.kernels"]}
    return funcs, meta


def main(old, new):
    with tempfile.TemporaryDirectory() as tmp:
        f0, m0 = kernels(old, os.path.basename(new), tmp, "old")
        f1, m1 = kernels(new, os.path.basename(new), tmp, "new")
    only = sorted(set(f0) ^ set(f1))
    bodies = sorted(k for k in set(f0) & set(f1) if f0[k] != f1[k])
    metas = sorted(k for k in set(m0) | set(m1) if m0.get(k) != m1.get(k))
    print(f"{len(f0)} / {len(f1)} kernel functions; in one only: {len(only)}; differing bodies: {len(bodies)}; "
          f"differing metadata entries: {len(metas)} of {len(m0)} / {len(m1)}")
    for k in only + bodies + metas:
        print("  ", k)
    return 1 if only or bodies or metas else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
