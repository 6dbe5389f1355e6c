"""Build librscotr.so (HIP kernels + C ABI) in-tree for gfx950.

`python -m rscotr_amd.build` or `rscotr_amd.build.build_library()`. hipcc cross-compiles
without a GPU; the resulting .so is git-ignored but travels with the tree to the GPU box.
"""
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librscotr.so")
STAMP = os.path.join(HERE, "librscotr.so.stamp")
ARCH = "gfx950"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-fast-math",
         "-Wno-unused-result"]
# host-only sources (bit-exact fp64 restatements, e.g. the LSAP solver) must not be FMA-contracted
HOST_FLAGS = ["-ffp-contract=off"]
# Kernels that fit their register budget with little to spare (csrc/gemm_split_body.h, h3_two_tiles: 246 - 249 of 256 VGPRs at two
# wavefronts per SIMD): their sources are compiled with the resource-usage remark, and the build fails if one of them spills.
REMARK_FLAGS = ["-Rpass-analysis=kernel-resource-usage"]
# (det_loss.hip: the per-kind box losses carry a gradient per corner through the IoU terms — CIoU's is the widest)
NO_SCRATCH = {"gemm_h3.hip": ("gemm_h3_128_kernel",), "gemm_group.hip": ("gemm_h3_group_kernel",),
              "det_loss.hip": ("box_loss_kernel", "match_cost_kernel", "qfl_sum_kernel")}


def scratch_report(remarks, names):
    """{kernel: bytes of scratch per lane} of the kernels whose mangled name holds one of `names`, from hipcc's
    kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in remarks.splitlines():
        if "Function Name:" in line:
            cur = line.split("Function Name:")[1].split()[0]
        elif "ScratchSize [bytes/lane]:" in line and cur is not None and any(n in cur for n in names):
            out[cur] = int(line.split("ScratchSize [bytes/lane]:")[1].split()[0])
    return out


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)
                  if f.endswith(".hip") or f.endswith(".cpp"))


def _digest():
    h = hashlib.sha256()
    for p in _sources() + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + \
            [os.path.join(HERE, "..", "include", "rscotr.h")]:
        h.update(p.encode())
        with open(p, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(FLAGS + HOST_FLAGS).encode())
    return h.hexdigest()


def find_hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def build_library(force=False, verbose=True):
    """Compile every source under csrc/ into one shared object. Returns the .so path."""
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(STAMP):
        with open(STAMP) as fh:
            if fh.read().strip() == dig:
                return LIB
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build librscotr.so")
    objs = []
    objdir = os.path.join(HERE, "_obj")
    os.makedirs(objdir, exist_ok=True)
    procs = []
    hdr = hashlib.sha256()
    for h in sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + \
            [os.path.join(HERE, "..", "include", "rscotr.h")]:
        with open(h, "rb") as fh:
            hdr.update(fh.read())
    for src in _sources():
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        extra = HOST_FLAGS if src.endswith(".cpp") else REMARK_FLAGS if os.path.basename(src) in NO_SCRATCH else []
        # per-object stamp: a source whose text, headers and flags are unchanged keeps its object
        with open(src, "rb") as fh:
            odig = hashlib.sha256(fh.read() + hdr.digest() + " ".join(FLAGS + extra).encode()).hexdigest()
        ostamp = obj + ".stamp"
        if not force and os.path.exists(obj) and os.path.exists(ostamp) and open(ostamp).read().strip() == odig:
            continue
        with open(ostamp, "w") as fh:
            fh.write(odig)
        cmd = [hipcc, f"--offload-arch={ARCH}", *FLAGS, *extra, "-x", "hip", "-c", src, "-o", obj,
               "-I", CSRC, "-I", os.path.join(HERE, "..", "include")]
        if verbose:
            print("[rscotr build]", " ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            os.remove(os.path.join(objdir, os.path.basename(src) + ".o.stamp"))
            raise RuntimeError(f"hipcc failed on {src}:\n{out.decode()}")
        names = NO_SCRATCH.get(os.path.basename(src))
        if names:
            report = scratch_report(out.decode(), names)
            spilled = {k: v for k, v in report.items() if v}
            if not report or spilled:
                os.remove(os.path.join(objdir, os.path.basename(src) + ".o.stamp"))
                raise RuntimeError(f"{src}: kernels that must not use scratch do (bytes per lane: {spilled}), or no resource-usage "
                                   f"remark was found for {names}: see h3_two_tiles in csrc/gemm_split_body.h")
    cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", *objs, "-ldl", "-o", LIB]
    if verbose:
        print("[rscotr build]", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(STAMP, "w") as fh:
        fh.write(dig)
    return LIB


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(LIB)
