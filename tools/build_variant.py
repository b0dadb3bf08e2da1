"""Development aid: build libredmax_hip with ONE kernel translation unit recompiled under extra flags, as
redmax_amd/variants/libredmax_hip_<name>.so (the other objects come from build/, i.e. run __graft_entry__.build() first).

    python tools/build_variant.py <name> [--part part_plain] [--np 32] [--no-ilp] -- <extra hipcc flags, e.g. -DRMX_VAR_X=1 -mllvm -foo>

--part names a row of __graft_entry__.HIP_UNITS by its source file (with or without .hip); --np picks the size of a multi-size
row.  The unit's own flags, the object list and the link line come from that table.  A part file defines RMX_SYNC / RMX_CONSTS under #ifndef, so a variant overrides them with plain -D.

tools/variant_bench.py times every variant in that directory on the GPU box (the .so files travel with the snapshot)."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        i = argv.index("--")
        argv, extra = argv[:i], argv[i + 1:]
    ap = argparse.ArgumentParser()
    ap.add_argument("name")
    ap.add_argument("--np", type=int, default=32, help="size of a multi-size row (ignored by a part that fixes its own)")
    ap.add_argument("--part", default="part_plain", help="source file of the unit (a row of __graft_entry__.HIP_UNITS)")
    ap.add_argument("--no-vform", action="store_true")
    ap.add_argument("--no-ilp", action="store_true", help="drop -amdgpu-sched-strategy=max-ilp where the in-tree build uses it")
    ap.add_argument("--host", action="store_true", help="also recompile the host unit under the extra flags (rmx_select.h chooses the kernel there)")
    ap.add_argument("--asm", action="store_true", help="also write the device assembly to build/isa/var_<name>.s")
    a = ap.parse_args(argv)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = a.part if a.part.endswith(".hip") else a.part + ".hip"
    jobs = ge.hip_jobs()
    rows = [j for j in ge.hip_jobs(ilp=not a.no_ilp, vform=not a.no_vform) if j[0] == src]
    if not rows:
        raise SystemExit("no unit %s in __graft_entry__.HIP_UNITS" % src)
    pick = [j for j in rows if len(rows) == 1 or j[1] == a.np]
    if not pick:
        raise SystemExit("%s is not built for --np %d (sizes: %s)" % (src, a.np, ", ".join(str(j[1]) for j in rows)))
    _, _, in_tree_obj, unit = pick[0]
    flags = ge.hip_base_flags()
    vdir = os.path.join(ROOT, "build", "variants")
    os.makedirs(vdir, exist_ok=True)
    obj = os.path.join(vdir, "%s.o" % a.name)
    tu = unit + extra + [os.path.join(ge.CSRC, src)]
    procs = [subprocess.Popen([hipcc] + flags + ["-c", "-o", obj] + tu)]
    if a.asm:
        os.makedirs(os.path.join(ROOT, "build", "isa"), exist_ok=True)
        procs.append(subprocess.Popen([hipcc] + flags + ["-S", "--cuda-device-only", "-o", os.path.join(ROOT, "build", "isa", "var_%s.s" % a.name)] + tu,
                                      stderr=subprocess.DEVNULL))
    if any(p.wait() != 0 for p in procs):
        raise SystemExit("hipcc failed")
    swap = {in_tree_obj: obj}
    if a.host:
        host = [j for j in jobs if j[0] == "redmax_hip.hip"][0]
        swap[host[2]] = os.path.join(vdir, "%s_host.o" % a.name)
        subprocess.check_call([hipcc] + flags + host[3] + extra + ["-c", "-o", swap[host[2]], os.path.join(ge.CSRC, host[0])])
    out = os.path.join(ROOT, "redmax_amd", "variants", "libredmax_hip_%s.so" % a.name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", out] + [swap.get(j[2], j[2]) for j in jobs])
    print(out)


main()
