"""The texture instances of the shade kernels next to their untextured counterparts of the same compile (no GPU: hipcc
cross-compiles gfx950, tools/resreport.py).

Every texture instance exists and runs without scratch; every kernel instance that existed before textures (the names in
tests/golden/kernel_names_before_textures.txt, taken from the parent's compile) is still there under its old name, with no
fewer waves per SIMD, no more scratch and no more LDS than its row of that compile (tests/golden/kernel_rows_before_textures.json:
VGPRs, AGPRs, scratch, waves, LDS; when it was recorded every row was equal in full, and a row that differs in any column is
printed); and the occupancy of each texture instance is printed beside its counterpart's (DESIGN.md section 3 "Textures" records the pairs; a
drop is stated there, not hidden).  The yardstick is the untextured kernel of this very compile, not a number fixed here."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

B = ("false", "true")


def counterpart(name):
    """The untextured instance that shades the same scenes in the same mode."""
    kernel, args = name.split("<")
    a = args.rstrip(">").split(", ")
    if kernel == "k_shade_tex":           # <INST, ABVH, ENV>
        return f"k_shade_env<{a[0]}, {a[1]}>" if a[2] == "true" else f"k_shade<0, true, {a[0]}, {a[1]}, false>"
    mesh, env = a[2] == "true", a[3] == "true"   # k_shade_nee_tex<INST, ABVH, MESHL, ENV>
    return "k_shade_nee" + ("_mesh" if mesh else "") + ("_env" if env else "") + f"<{a[0]}, {a[1]}>"


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_texture_instances_exist_without_scratch_beside_the_old_ones():
    import resreport
    rows = {r["name"]: r for r in resreport.report()}
    old = open(os.path.join(ROOT, "tests", "golden", "kernel_names_before_textures.txt")).read().split("\n")
    missing = [n for n in old if n and n not in rows]
    assert not missing, missing
    before = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_rows_before_textures.json")))
    assert sorted(before) == sorted(n for n in old if n)
    worse = []
    for n, b in sorted(before.items()):
        r = {k: rows[n][k] for k in b}
        if r != b:
            print(f"{n}: {b} -> {r}")
        if r["occ"] < b["occ"] or r["scratch"] > b["scratch"] or r["lds"] > b["lds"]:
            worse.append((n, b, r))
    assert not worse, worse
    want = [f"k_shade_tex<{i}, {a}, {e}>" for i in B for a in B for e in B]
    want += [f"k_shade_nee_tex<{i}, {a}, {m}, {e}>" for i in B for a in B for m in B for e in B]
    tex = {n: r for n, r in rows.items() if n.startswith(("k_shade_tex", "k_shade_nee_tex"))}
    assert sorted(tex) == sorted(want)
    for n in ("k_texture_eval", "k_hit_uv"):
        assert n in rows and rows[n]["scratch"] == 0, n
    print()
    for n in want:
        r, c = rows[n], rows[counterpart(n)]
        print(f"{n:48s} vgpr {r['vgpr']:3d} occ {r['occ']}   | {counterpart(n):40s} vgpr {c['vgpr']:3d} occ {c['occ']}")
        assert r["scratch"] == 0, (n, r)
