"""CPU check of the engine library's build recipe (blokus_rl_amd/csrc/Makefile): every side build (an
OUT / EXTRA / EXTRA_<stem> variant, each stamp target) compiles the default target's sources by the
default target's own commands, with only the output paths replaced and the variant's flags added.
Reads `make -n -B`; compiles nothing."""
import os
import shlex
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "blokus_rl_amd", "csrc")
PROBE = "-DBK_RECIPE_PROBE=1"
# target -> (library under OUT, its define)
STAMP_TARGETS = {
    "diag": ("diag/libblokus_hip_diag.so", "-DBK_STAMPS"),
    "stamps": ("exp/libst.so", "-DBK_WINO_STAMP=1"),
    "lnstamps": ("exp/liblnst.so", "-DBK_LN_STAMP=1"),
    "vecstamps": ("exp/libvecst.so", "-DBK_VEC_STAMP=1"),
}


def without_output(tokens):
    """(the command without its `-o PATH`, PATH)"""
    i = tokens.index("-o")
    return tokens[:i] + tokens[i + 2:], os.path.normpath(os.path.join(CSRC, tokens[i + 1]))


def recipe(*make_args):
    """The dry run's compiler commands: {source: (command without -o, object)}, (link command
    without -o and objects, library, objects)."""
    env = {k: v for k, v in os.environ.items() if k not in ("MAKEFLAGS", "MFLAGS", "MAKELEVEL")}
    out = subprocess.run(["make", "-n", "-B", *make_args], cwd=CSRC, env=env, check=True,
                         capture_output=True, text=True).stdout
    compiles, links = {}, []
    for line in out.splitlines():
        tokens = shlex.split(line)
        if not tokens or os.path.basename(tokens[0]) != "hipcc":
            continue
        cmd, target = without_output(tokens)
        if "-c" in cmd:
            assert cmd[-2] == "-c" and cmd[-1] not in compiles, line
            compiles[cmd[-1]] = (cmd, target)
        else:
            assert "-shared" in cmd, line
            objs = [os.path.normpath(os.path.join(CSRC, t)) for t in cmd if t.endswith(".o")]
            links.append(([t for t in cmd if not t.endswith(".o")], target, objs))
    assert len(links) == 1, out
    return compiles, links[0]


@pytest.fixture(scope="module")
def default():
    compiles, link = recipe()
    hip = [s for s in compiles if s.endswith(".hip")]
    assert len(hip) >= 18 and "tables.cpp" in compiles
    assert link[1] == os.path.join(ROOT, "blokus_rl_amd", "_lib", "libblokus_hip.so")
    return compiles, link


def check_variant(default, make_args, lib, added):
    """added(source) -> the flags this variant adds to that source's compile. Returns its object dir."""
    (d_compiles, (d_link, _, d_objs)), (compiles, (link, v_lib, objs)) = default, recipe(*make_args)
    assert sorted(compiles) == sorted(d_compiles)
    for src, (cmd, obj) in compiles.items():
        d_cmd = d_compiles[src][0]
        assert cmd == d_cmd[:-2] + added(src) + d_cmd[-2:], src
        assert os.path.basename(obj) == os.path.basename(d_compiles[src][1])
    assert "-fno-slp-vectorize" in compiles["conv.hip"][0]
    assert any(t.startswith("-pragma-unroll-threshold=") for t in compiles["leafnet_w3.hip"][0])
    assert link == d_link and v_lib == os.path.normpath(lib)
    assert sorted(objs) == sorted(obj for _, obj in compiles.values()) and len(set(objs)) == len(d_objs)
    obj_dirs = {os.path.dirname(o) for o in objs}
    assert len(obj_dirs) == 1 and obj_dirs != {os.path.dirname(d_objs[0])}
    return obj_dirs.pop()


def test_default_keeps_per_file_flags(default):
    compiles = default[0]
    carries = {src for src, (cmd, _) in compiles.items() if "-fno-slp-vectorize" in cmd}
    assert carries == {"conv.hip"}
    carries = {src for src, (cmd, _) in compiles.items() if any(t.startswith("-pragma-unroll-threshold=") for t in cmd)}
    assert carries == {"leafnet_w3.hip"}


def test_extra_reaches_every_hip_source(default, tmp_path):
    d = check_variant(default, [f"OUT={tmp_path}", f"EXTRA={PROBE}"], tmp_path / "libblokus_hip.so",
                      lambda src: [PROBE] if src.endswith(".hip") else [])
    assert d == str(tmp_path / "obj")


def test_extra_stem_reaches_one_source(default, tmp_path):
    check_variant(default, [f"OUT={tmp_path}", f"EXTRA_leafnet={PROBE}"], tmp_path / "libblokus_hip.so",
                  lambda src: [PROBE] if src == "leafnet.hip" else [])


def test_stamp_targets_are_the_default_plus_one_define(default, tmp_path):
    dirs = [check_variant(default, [target, f"OUT={tmp_path}"], tmp_path / lib,
                          lambda src, define=define: [define] if src.endswith(".hip") else [])
            for target, (lib, define) in STAMP_TARGETS.items()]
    assert len(set(dirs)) == len(dirs)  # no two variants share an object directory
    # the caller's flags travel into a stamp build, and its own OUT keeps the in-tree output names
    check_variant(default, ["lnstamps", f"EXTRA={PROBE}", f"EXTRA_leafnet={PROBE}2"],
                  os.path.join(ROOT, "blokus_rl_amd", "_lib", "exp", "liblnst.so"),
                  lambda src: ([PROBE, "-DBK_LN_STAMP=1"] if src.endswith(".hip") else [])
                  + ([PROBE + "2"] if src == "leafnet.hip" else []))
