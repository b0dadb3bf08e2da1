"""The build recipe is ONE table (__graft_entry__.HIP_UNITS): the objects, the compile commands, the link line and the dependency
list all derive from it, and so does tools/build_variant.py.  These checks read the table; none invokes the compiler."""
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NPS = (4, 8, 16, 32, 64)
# every object of the library: (source file, padded tree size or None)
EXPECTED = sorted(
    [("part_plain.hip", n) for n in NPS] + [("part_ct.hip", n) for n in NPS] + [("part_pf.hip", n) for n in NPS]
    + [("part_fullchain.hip", n) for n in (16, 32, 64)]
    + [("part_gconst64.hip", 64), ("part_ground32.hip", 32), ("part_w2_tree64.hip", 64), ("part_w2_chain32.hip", 32),
       ("part_pair32.hip", 32), ("part_adjhelp16.hip", 16)]
    + [("rmx_big.hip", None), ("redmax_hip.hip", None)], key=str)


def test_every_source_file_exists():
    for src, _, _, _ in ge.HIP_UNITS:
        assert os.path.isfile(os.path.join(ge.CSRC, src)), src


def test_every_part_file_is_in_the_table():
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ge.CSRC, "part_*.hip")))
    in_table = sorted(src for src, _, _, _ in ge.HIP_UNITS if src.startswith("part_"))
    assert on_disk == in_table


def test_object_paths_are_unique():
    objs = [obj for _, _, obj, _ in ge.hip_jobs()]
    assert len(objs) == len(set(objs))
    assert all(os.path.dirname(o) == ge.OBJ_DIR for o in objs)


def test_deps_cover_every_file_of_csrc():
    deps = set(ge.HIP_DEPS)
    for f in os.listdir(ge.CSRC):
        assert os.path.join(ge.CSRC, f) in deps, f
    for extra in (os.path.join(ROOT, "include", "redmax_hip.h"), os.path.join(ROOT, "include", "redmax_hip_profile.h"),
                  os.path.join(ROOT, "__graft_entry__.py")):
        assert extra in deps, extra


def test_units_and_sizes_are_the_librarys():
    assert sorted([(src, n) for src, n, _, _ in ge.hip_jobs()], key=str) == EXPECTED


def test_no_semantic_macro_on_the_command_line():
    # what a kernel object IS (its size apart, for the multi-size parts) is written in its source file, not passed by the build
    for src, n, _, unit in ge.hip_jobs():
        cmd = ge.hip_base_flags() + unit
        for macro in ("PART", "W2", "SYNC", "CONSTS", "GLOBAL_CONSTS"):
            assert not any(x.startswith("-DRMX_" + macro) for x in cmd), (src, n, cmd)
        defines = [x for x in unit if x.startswith("-D")]
        multi = sum(1 for s, _, _, _ in ge.hip_jobs() if s == src) > 1
        assert defines == (["-DRMX_NP=%d" % n] if multi else []), (src, n, defines)
