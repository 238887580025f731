"""The SGPR-into-VGPR spill hazard, gated on what the compiler emitted (no GPU).

Every unit of build.SOURCES is read back from its built object: the gfx950 code object is unbundled from the .hip_fatbin
section and each kernel's metadata (.sgpr_spill_count, .vgpr_spill_count, .private_segment_fixed_size) is read from its
notes.  A kernel of a unit compiled WITHOUT SPILL_SAFE (by the command stamp build.py writes beside the object) that
spills both kinds is exposed; the exposed set must be exactly tests/spill_exposed.py's EXPOSED, whose every entry has
an every-lane GPU case (tests/test_gpu_spill_lanes.py).  A newly exposed kernel fails here until it has one; an entry
that is no longer exposed fails as stale.

Also here: build.py rebuilds an object whose compile command changed (its flags), not only one older than its sources."""
import functools
import os
import re
import shutil
import subprocess

import pytest

import spill_exposed as sx
from mdp_playground_amd import build

LLVM = "/opt/rocm/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
_KEYS = ("name", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")


def _obj(unit):
    return os.path.join(build.CSRC, unit.replace(".hip", ".o"))


def _kernel_notes(text):
    """llvm-readelf --notes text -> [{name, sgpr_spill_count, vgpr_spill_count, private_segment_fixed_size}] per kernel
    (kernel-level keys only: the argument lists' .name entries are indented deeper)."""
    kernels, cur, inside = [], None, False
    for line in text.splitlines():
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if inside and line and not line.startswith(" "):
            inside = False
        if not inside:
            continue
        if line.startswith("  - "):
            cur = {}
            kernels.append(cur)
            line = "    " + line[4:]
        m = re.match(r"    \.([a-z_]+):\s+(\S+)\s*$", line)
        if m and cur is not None and m.group(1) in _KEYS:
            cur[m.group(1)] = m.group(2) if m.group(1) == "name" else int(m.group(2))
    return kernels


@functools.lru_cache(maxsize=None)
def _unit_kernels(unit, tmp):
    obj = _obj(unit)
    if not os.path.exists(obj):
        pytest.fail(f"{obj} is missing: run `python -m mdp_playground_amd.build` first")
    base = os.path.join(tmp, unit.replace(".hip", ""))
    for cmd in ([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, base + ".fatbin"],
                [f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + base + ".fatbin", "--targets=" + TARGET,
                 "--output=" + base + ".elf"]):
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (cmd, r.stdout)
    r = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", base + ".elf"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    ks = _kernel_notes(r.stdout)
    assert all(set(k) == set(_KEYS) for k in ks), (unit, [k for k in ks if set(k) != set(_KEYS)][:3])
    return tuple(tuple(k[x] for x in _KEYS) for k in ks)


def _stamp(unit):
    p = _obj(unit) + ".cmd"
    if not os.path.exists(p):
        pytest.fail(f"{p} is missing (an object built before build.py wrote command stamps): run `python -m mdp_playground_amd.build`")
    return open(p).read().split()


def _spill_safe(unit):
    return sx.SPILL_SAFE_FLAG in _stamp(unit)


def _demangle(names):
    cf = shutil.which("c++filt")
    if not cf:
        return list(names)
    return subprocess.run([cf], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()


@pytest.fixture(scope="module")
def inventory(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("codeobjects"))
    return {u: _unit_kernels(u, tmp) for u in build.SOURCES}


def _exposed(inventory):
    out = {}
    for unit, ks in inventory.items():
        if _spill_safe(unit):
            continue
        for name, sgpr, vgpr, scratch in ks:
            if sgpr > 0 and vgpr > 0:
                key = sx.parse_mangled(name)
                assert key[1] is not None, name
                assert key not in out, (key, unit, out.get(key))
                out[key] = (unit, scratch, sgpr, vgpr, name)
    return out


def test_spill_safe_units_are_built_with_the_flag():
    """The units that must not park SGPRs in VGPR lanes really were compiled with SPILL_SAFE -- read from the command that
    built each object, not inferred from metadata (an SGPR spill count looks the same whether it goes to lanes or memory)."""
    assert sx.SPILL_SAFE_FLAG in build.SPILL_SAFE
    assert sorted(u for u, f in build.EXTRA_FLAGS.items() if sx.SPILL_SAFE_FLAG in f) == sorted(sx.SPILL_SAFE_UNITS)
    for u in sx.SPILL_SAFE_UNITS:
        assert u in build.SOURCES, u
        assert _spill_safe(u), (u, " ".join(_stamp(u)))
    for u in set(build.SOURCES) - set(sx.SPILL_SAFE_UNITS):
        assert not _spill_safe(u), u      # (a unit with the flag belongs in the pinned list)


def test_every_unit_yields_a_code_object(inventory):
    for u in build.SOURCES:
        assert inventory[u], u
    default = sum(len(ks) for u, ks in inventory.items() if u not in sx.SPILL_SAFE_UNITS)
    assert default >= 500, default
    assert sum(len(ks) for ks in inventory.values()) >= 800


def test_spill_exposed_kernels_match_the_reviewed_table(inventory):
    """Kernels of default-flag units with both SGPR and VGPR spills == the keys of EXPOSED, in both directions."""
    found = _exposed(inventory)
    new = sorted(set(found) - set(sx.EXPOSED))
    stale = sorted(set(sx.EXPOSED) - set(found))
    lines = []
    for key, dm in zip(new, _demangle([found[k][4] for k in new])):
        unit, scratch, sgpr, vgpr, _ = found[key]
        lines.append(f"  NEW   {sx.describe(key)}  [{unit}: {scratch} B scratch, {sgpr} SGPR / {vgpr} VGPR spills]  {dm}")
    lines += [f"  STALE {sx.describe(k)} (case {sx.EXPOSED[k]}): no longer exposed -- drop the entry" for k in stale]
    assert not lines, ("exposed kernels differ from tests/spill_exposed.py EXPOSED (a new one needs an every-lane GPU case, "
                       "tests/test_gpu_spill_lanes.py):\n" + "\n".join(lines))
    assert len(found) == len(sx.EXPOSED)


def test_kernel_note_parser_reads_kernel_level_keys_only():
    text = """amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .name:           a
        .offset:         0
    .name:           _ZN4mdpp1kILi3ELb1ELin2EEEvv
    .private_segment_fixed_size: 420
    .sgpr_spill_count: 38
    .vgpr_spill_count: 104
  - .args:           []
    .name:           _ZN4mdpp1jEvv
    .private_segment_fixed_size: 0
    .sgpr_spill_count: 0
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""
    ks = _kernel_notes(text)
    assert ks == [dict(name="_ZN4mdpp1kILi3ELb1ELin2EEEvv", private_segment_fixed_size=420, sgpr_spill_count=38, vgpr_spill_count=104),
                  dict(name="_ZN4mdpp1jEvv", private_segment_fixed_size=0, sgpr_spill_count=0, vgpr_spill_count=0)]
    assert sx.parse_mangled(ks[0]["name"]) == ("k", (3, 1, -2))
    assert sx.parse_mangled(ks[1]["name"]) == ("j", ())


def test_dispatched_names_parse_to_the_mangled_keys():
    assert sx.parse_dispatched("k_continuous_rollout_fast<D=12,ORDER=2,NREL=4,NOISE=1,HELPER=1,GEN=0,PHILOX=0,NPROD=2>") == \
        ("k_continuous_rollout_fast", (12, 2, 4, 1, 1, 0, 0, 2, 0, 0, 0))
    assert sx.parse_dispatched("k_continuous_step1<D=12,ORDER=2,NREL=12,NOISE=1,GEN=1,PHILOX=0,PAR=1>") == \
        ("k_continuous_rollout_fast", (12, 2, 12, 1, 0, 1, 0, 1, 1, 1, 0))
    # (the mangled spelling of the first: int literals Li, bool literals Lb)
    assert sx.parse_mangled("_ZN4mdpp25k_continuous_rollout_fastILi12ELi2ELi4ELb1ELb1ELb0ELb0ELi2ELb0ELb0ELb0EEEvNS_14ContinuousArgsEiPKfPfS4_PhS5_S4_") == \
        ("k_continuous_rollout_fast", (12, 2, 4, 1, 1, 0, 0, 2, 0, 0, 0))


# --- build.py: a changed compile command makes the object stale

@pytest.fixture
def fake_tree(tmp_path, monkeypatch):
    csrc = tmp_path / "pkg" / "csrc"      # (HEADERS reach ../../include/mdpp.h: tmp_path/include)
    csrc.mkdir(parents=True)
    for s in build.SOURCES + build.HEADERS:
        p = csrc / s
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_text("// dummy\n")
    calls = []

    class Done:
        returncode, stdout = 0, ""

    def fake_run(cmd, **kw):
        calls.append(list(cmd))
        out = cmd[cmd.index("-o") + 1]
        with open(out, "w") as f:
            f.write("x")
        return Done()

    monkeypatch.setattr(build, "CSRC", str(csrc))
    monkeypatch.setattr(build, "OUT", str(csrc / "libmdpp_hip.so"))
    monkeypatch.setattr(build, "_hipcc", lambda: "/bin/hipcc-stub")
    monkeypatch.setattr(build.subprocess, "run", fake_run)
    return csrc, calls


def _compiled(calls):
    return sorted(os.path.basename(c[c.index("-c") + 1]) for c in calls if "-c" in c)


def _linked(calls):
    return [c for c in calls if "-shared" in c]


def test_stale_objects_rebuild_when_their_compile_flags_change(fake_tree, monkeypatch):
    csrc, calls = fake_tree
    build.build()
    assert _compiled(calls) == sorted(build.SOURCES) and len(_linked(calls)) == 1
    assert all(os.path.exists(str(csrc / s.replace(".hip", ".o.cmd"))) for s in build.SOURCES)
    calls.clear()
    build.build()
    assert calls == []              # nothing changed: nothing compiled, nothing linked
    unit = "mdpp_continuous.hip"
    flags = dict(build.EXTRA_FLAGS)
    flags[unit] = []                # (e.g. SPILL_SAFE dropped from the round-6 kernel's unit)
    monkeypatch.setattr(build, "EXTRA_FLAGS", flags)
    build.build()
    assert _compiled(calls) == [unit] and len(_linked(calls)) == 1
    assert sx.SPILL_SAFE_FLAG not in open(str(csrc / "mdpp_continuous.o.cmd")).read()
    calls.clear()
    build.build()
    assert calls == []
    # a source newer than its object still rebuilds it (and only it); a missing stamp counts as a changed command
    t = os.path.getmtime(str(csrc / "mdpp_grid.hip")) - 10
    os.utime(str(csrc / "mdpp_grid.o"), (t, t))
    os.remove(str(csrc / "mdpp_post.o.cmd"))
    build.build()
    assert _compiled(calls) == ["mdpp_grid.hip", "mdpp_post.hip"] and len(_linked(calls)) == 1
