"""Build the HIP engine in-tree for gfx950:  python -m iaf_amd.build [--force]
Output: iaf_amd/_lib/libiaf_hip.so (git-ignored; travels to the GPU box with the snapshot).

The conv kernels are instantiated once per launch shape, and the one-launch step once per part, each in its own translation
unit (e.g. csrc/iaf_conv_inst.hip with -DIAF_PXT/-DIAF_WCO/-DIAF_KS); the units compile in parallel.  Which shapes and parts
exist is csrc/iaf_variants.def, read here and included by the engine."""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
# IAF_BUILD_TAG=<tag> (with IAF_EXTRA_CFLAGS) builds an experiment library next to the product one, in _lib_<tag>/;
# load it with IAF_HIP_LIB=<path> (iaf_amd/_capi.py).  The product library is always _lib/libiaf_hip.so.
_TAG = os.environ.get("IAF_BUILD_TAG", "")
LIBDIR = os.path.join(HERE, "_lib" + ("_" + _TAG if _TAG else ""))
OBJDIR = os.path.join(LIBDIR, "obj")
OUT = os.path.join(LIBDIR, "libiaf_hip.so")
VARIANTS = os.path.join(CSRC, "iaf_variants.def")


def _read_variants(path=VARIANTS):
    """{macro: [argument tuple, ...]} in file order; any line that is not a comment, an entry or the file's own macro plumbing is an error"""
    arity = {"IAF_CONV": 3, "IAF_BF3": 4, "IAF_BF3P": 5, "IAF_STEP_PART": 1}
    out = {k: [] for k in arity}
    for n, line in enumerate(open(path), 1):
        line = line.strip()
        if not line or line.startswith("//") or re.fullmatch(r"#(ifndef|undef) IAF_\w+|#define IAF_\w+\([\w, ]*\)|#endif", line):
            continue
        m = re.fullmatch(r"(IAF_\w+)\(([\d, ]*)\)", line)
        args = tuple(int(a) for a in m.group(2).split(",")) if m else ()
        if not m or len(args) != arity.get(m.group(1), -1):
            raise ValueError("%s:%d: not a variant entry: %r" % (path, n, line))
        out[m.group(1)].append(args)
    return out


_V = _read_variants()
SHAPES = _V["IAF_CONV"]                # exact-fp32 conv: (pxt, wco, ks)
BF3_SHAPES = _V["IAF_BF3"]             # bf16x3 masked conv: (ppw, pxt, ks, wco)
BF3_PLAIN_SHAPES = _V["IAF_BF3P"]      # 9-tap plain conv: (ppw, pxt, ks, wco, strided / deconv forms compiled)
STEP_PARTS = [p for (p,) in _V["IAF_STEP_PART"]]
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
CFLAGS += os.environ.get("IAF_EXTRA_CFLAGS", "").split()       # dev experiments only (e.g. -DIAF_EXP_NOREFILL)
HEADERS = [os.path.join(ROOT, "include", "iaf_hip.h")] + sorted(
    os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp"))   # fallback: no dependency file yet -> every header counts


def _units():
    units = [(os.path.join(CSRC, "iaf_engine.hip"), os.path.join(OBJDIR, "iaf_engine.o"), []),
             # the entry points that take no stack and no conv: optimiser, guard, summaries, noise source, dataset, state snapshot
             (os.path.join(CSRC, "iaf_train_services.hip"), os.path.join(OBJDIR, "iaf_train_services.o"), []),
             # ... and the model's own: its two ends around the layer stack, the objective side, the elementwise pieces of the init pass
             (os.path.join(CSRC, "iaf_model_ops.hip"), os.path.join(OBJDIR, "iaf_model_ops.o"), []),
             # host-only: the RCCL gradient exchange (librccl is dlopen'ed at run time, no link dependency)
             (os.path.join(CSRC, "iaf_comm.cpp"), os.path.join(OBJDIR, "iaf_comm.o"), ["-x", "hip"]),
             # the weight gradient on the bf16 matrix cores (transposing LDS reads)
             (os.path.join(CSRC, "iaf_wgrad_bf3.hip"), os.path.join(OBJDIR, "iaf_wgrad_bf3.o"), [])]
    for pxt, wco, ks in SHAPES:
        units.append((os.path.join(CSRC, "iaf_conv_inst.hip"), os.path.join(OBJDIR, "iaf_conv_%d_%d_%d.o" % (pxt, wco, ks)),
                      ["-DIAF_PXT=%d" % pxt, "-DIAF_WCO=%d" % wco, "-DIAF_KS=%d" % ks]))
    for ppw, pxt, ks, wco in BF3_SHAPES:
        units.append((os.path.join(CSRC, "iaf_conv_bf3_inst.hip"), os.path.join(OBJDIR, "iaf_bf3_%d_%d_%d_%d.o" % (ppw, pxt, ks, wco)),
                      ["-DIAF_PPW=%d" % ppw, "-DIAF_PXT=%d" % pxt, "-DIAF_KS=%d" % ks, "-DIAF_WCO=%d" % wco]))
    for ppw, pxt, ks, wco, s2 in BF3_PLAIN_SHAPES:
        units.append((os.path.join(CSRC, "iaf_conv_bf3_plain_inst.hip"), os.path.join(OBJDIR, "iaf_bf3p_%d_%d_%d_%d.o" % (ppw, pxt, ks, wco)),
                      ["-DIAF_PPW=%d" % ppw, "-DIAF_PXT=%d" % pxt, "-DIAF_KS=%d" % ks, "-DIAF_WCO=%d" % wco, "-DIAF_S2=%d" % s2]))
    # accumulators in architectural VGPRs: left to itself the register allocator puts them in AGPRs and rotates them through
    # VGPR copies inside the K loop (48 v_accvgpr moves per 162 MFMAs)
    for part in STEP_PARTS:
        units.append((os.path.join(CSRC, "iaf_step_fused_inst.hip"), os.path.join(OBJDIR, "iaf_step_fused_%d.o" % part),
                      ["-mllvm", "-amdgpu-mfma-vgpr-form=1", "-DIAF_FUSED_PART=%d" % part]))
    return units


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any((not os.path.exists(d)) or os.path.getmtime(d) > t for d in deps)


def _deps(obj, src):
    """headers the unit actually includes (hipcc -MD wrote obj + '.d' at the last compile), else every project header"""
    d = obj + ".d"
    if not os.path.exists(d):
        return [src, VARIANTS] + HEADERS
    words = open(d).read().replace("\\\n", " ").split()
    mine = [w for w in words[1:] if w.startswith(ROOT) or not os.path.isabs(w)]      # project files only (not /opt/rocm)
    return [src, VARIANTS] + mine          # (the variant list also sets units' -D flags)


def build(force=False, verbose=True, jobs=None):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    os.makedirs(OBJDIR, exist_ok=True)
    todo = []
    for src, obj, defs in _units():
        if force or _stale(obj, _deps(obj, src)):
            todo.append([hipcc] + CFLAGS + defs + ["-MD", "-MF", obj + ".d", "-c", src, "-o", obj])
    if todo:
        # MAX_JOBS: the CPUs this process may use, where os.cpu_count() reports a larger shared host
        jobs = jobs or min(len(todo), int(os.environ.get("MAX_JOBS") or 0) or os.cpu_count() or 4)
        if verbose:
            print("compiling %d translation unit(s) for gfx950 with %d job(s)" % (len(todo), jobs), flush=True)
        with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
            for cmd, rc in zip(todo, ex.map(lambda c: subprocess.run(c).returncode, todo)):
                if rc != 0:
                    raise RuntimeError("hipcc failed: " + " ".join(cmd))
    objs = [obj for _, obj, _ in _units()]
    if force or todo or _stale(OUT, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-ldl", "-o", OUT]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
