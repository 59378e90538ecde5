"""gpu_build 2 (the Morton octree builder, csrc/bvh_gpu.hip prt_gpu_bvh8_build: k_morton, k_split, k_boxes, k_quantize,
k_records) held to tests/octree_replay.py's numpy restatement, field by field, up to node and record numbering (child_base
and tri_base come from atomics).  The closest hit does not depend on the tree, so hits, validity and tightness cannot see a
wrong Morton digit, a child in the wrong octant slot, a level skipped wrongly or a range split one element off; this can.
One Init on a 16 x 16 film per input; the inputs are the smallest that reach each path (builder_inputs.OCTREE_INPUTS,
whose conditions tests/test_octree_replay.py checks without a GPU)."""
import numpy as np
import pytest

import builder_inputs as bi
import octree_replay as oc
import ploc_replay as pr

pytestmark = pytest.mark.gpu
_cache = {}   # name -> what builder_inputs.prepare made of the input: built once


@pytest.mark.parametrize("name", list(bi.OCTREE_INPUTS))
def test_morton_builder_tree_equals_the_replay(name):
    if name not in _cache:
        _cache[name] = bi.prepare(bi.OCTREE_INPUTS[name][0]())
    c = _cache[name]
    r = bi.build(c["scene"], 2)   # (asserts built_on_device == 1: a fall-back to the host builder is a wrong input, not a pass)
    assert r.bvh_info().built_on_device == 1
    n8, tris, n_prims = bi.check_tree(r, c)
    info = {}
    want = oc.replay(c["tv"], *pr.centroid_bounds(c["tv"]), info=info)
    print(f"{name}: {len(c['tv'])} triangles, {len(n8)} nodes, {info}", flush=True)
    assert len(np.unique(want["child"][want["child"] >= 0])) == len(n8) - 1
    pr.assert_same_tree(pr.canonical(n8, tris, n_prims), want, f"{name}, gpu_build 2")
