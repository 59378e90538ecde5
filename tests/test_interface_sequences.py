"""The model and the generator of tests/interface_sequences.py, without a GPU.

1. What the committed campaign (CAMPAIGN_SEED, CAMPAIGN_CASES: the cases tests/test_gpu_fuzz.py runs) covers, counted from the
   operation lists and the model alone.  The floors are conditions, not measurements: a generator change that loses one of
   them fails here, on any machine, before a GPU sees it.
2. The model against the oracle: a sequence rendered in one oracle call equals the same sequence rendered in the model's
   chunks, byte for byte, ray for ray.
3. The three verdicts on hand-written sequences."""
import numpy as np

import util  # noqa: F401  (puts the repository root on sys.path)
import interface_sequences as iseq
from interface_sequences import EITHER, MUST, MUST_NOT


def test_the_campaign_covers_the_interface():
    c = iseq.coverage()
    kinds = ["render", "reinit"] + [k for k in iseq.SETTER_OPS if k != "reinit"] + ["query:" + q for q in iseq.QUERIES] + ["excursion"]
    short = {k: c["kinds"].get(k, 0) for k in kinds if c["kinds"].get(k, 0) < 5}
    assert short == {}, short                                   # every operation kind at least 5 times
    assert c["equal"] >= 30 and c["equal_query"] >= 10, c        # batches after a batch of equal size, no setter between; with a query between
    assert c["big"] >= 8, c                                      # batches of 64 samples or more
    assert all(c["after"][k] >= 6 for k in ("refit", "instances", "set_film", "max_depth")), c["after"]
    assert all(c["excursions"].get(e, 0) >= 3 for e in iseq.EXCURSIONS), c["excursions"]
    assert c["groups"] >= 8, c["groups"]


def test_the_generator_is_a_function_of_seed_and_case():
    for case in (0, 7, 39):
        assert iseq.generate(iseq.CAMPAIGN_SEED, case) == iseq.generate(iseq.CAMPAIGN_SEED, case)
    assert iseq.generate(iseq.CAMPAIGN_SEED, 1) != iseq.generate(iseq.CAMPAIGN_SEED, 2)
    head, ops = iseq.generate(iseq.CAMPAIGN_SEED, 0)
    assert ops[0][0] == "init" and ops[-1][0] == "render"
    for case in range(iseq.CAMPAIGN_CASES):                      # a group takes the setters only; films stay within 96 x 48
        head, ops = iseq.generate(iseq.CAMPAIGN_SEED, case)
        assert not head["group"] or not any(op[0] in ("query", "excursion", "set_film") for op in ops), case
        assert all(op[2] <= 96 and op[3] <= 48 for op in ops if op[0] == "init"), case
        assert all(op[1] <= 96 and op[2] <= 48 for op in ops if op[0] == "set_film"), case
        assert all(65 <= op[2] <= 5000 for op in ops if op[0] == "query"), case


def _model(W=40, H=24, S=1, scene=None, kind="directed", sampling=None):
    m = iseq.Model(iseq.DEPTH, iseq.SEED)
    m.init(scene or iseq.directed_scene(), kind, W, H, iseq.camera(W, H, iseq.CAM_POS), use_bvh=True)
    if sampling:
        m.set_sampling(*sampling)
    m.set_samples_in_flight(S)
    return m


def test_chunks_equal_one_oracle_call():
    """70 samples as render calls of 1, 3, 64 and 2 (and again split by samples in flight) against ONE oracle call of 70."""
    for sampling in (None, (0, 2, 1.5), (1, 0, 0.0)):
        m = _model(sampling=sampling)
        for k, sif in ((1, 1), (3, 2), (64, 64), (2, 5)):
            m.set_samples_in_flight(sif)
            m.render(k)
        one = _model(sampling=sampling)
        acc, wts, rays = one.osc.render(one.cam.desc(), 40, 24, spp=70, first_sample=0, max_depth=iseq.DEPTH, seed=iseq.SEED, iterative=True,
                                        use_bvh=True, n_threads=8, sampling=one.sp)
        assert m.acc.tobytes() == acc.tobytes() and m.wts.tobytes() == wts.tobytes() and m.rays == rays and m.fi == 70
        assert (wts == 70).all() and len(np.unique(acc.reshape(-1, 3), axis=0)) > 100      # a picture
        assert [b["size"] for b in m.log] == [1, 2, 1, 64, 2]
    # a Refit between two chunks: each chunk is of the scene it was rendered with
    m = _model()
    m.render(2)
    m.refit(iseq.directed_scene(displaced=True))
    m.render(3)
    a = _model()
    acc, wts, r1 = a.osc.render(a.cam.desc(), 40, 24, spp=2, max_depth=iseq.DEPTH, seed=iseq.SEED, iterative=True, use_bvh=True)
    b = _model(scene=iseq.directed_scene(displaced=True))
    acc, wts, r2 = b.osc.render(b.cam.desc(), 40, 24, spp=3, first_sample=2, max_depth=iseq.DEPTH, seed=iseq.SEED, iterative=True, use_bvh=True,
                                accum=acc, weights=wts)
    assert m.acc.tobytes() == acc.tobytes() and m.rays == r1 + r2
    assert m.acc.tobytes() != _replayed(5).tobytes()


def _replayed(k):
    m = _model()
    m.render(k)
    return m.acc


def _verdicts(recs):
    return [b["verdict"] for b in recs]


def test_the_three_verdicts():
    m = _model(S=3)
    assert _verdicts(m.render(3)) == [MUST_NOT]                  # nothing is held yet (and Init is a setter)
    assert _verdicts(m.render(9)) == [MUST, MUST, MUST]
    assert _verdicts(m.render(10)) == [MUST, MUST, MUST, MUST_NOT]   # a shorter last batch has a key of its own
    assert _verdicts(m.render(3)) == [MUST_NOT]
    for q in ("closest_hit", "radiance", "display", "stats"):
        m.query(q)
    m.clear()
    rec = m.render(3)[0]
    assert rec["verdict"] == MUST and rec["queries"] == ("closest_hit", "radiance", "display", "stats") and rec["setters"] == ()
    m.set_param("radiance_chunk", 1)                              # any prt_set_param bumps a generation
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, MUST]
    assert m.measure("measure_traversal")["verdict"] == MUST_NOT  # an instrumented batch neither reuses nor leaves a stage
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, MUST]
    m.set_max_depth(4)                                            # no setter, but in the key
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, MUST]
    m.set_film_statistics(True)
    m.set_film_statistics(True)                                   # (the second call changes nothing)
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, MUST]
    assert _verdicts(m.adaptive(3, 3, 6, 1)) == [MUST, MUST_NOT] and not m.known
    m.clear()
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, MUST] and m.known
    m.set_sampling(1, 0, 0.0)                                     # jitter: never
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, MUST_NOT]
    m.set_sampling(0, 2, 0.0)                                     # roulette: the planner's business
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, EITHER]
    m.set_sampling(0, 0, 0.0)
    m.set_param("primary_reuse", 0)
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, MUST_NOT]
    m.set_param("primary_reuse", 1)
    m.set_param("primary_walk", 0)                                # one walk per sample: offered to one-sample batches only
    assert _verdicts(m.render(3)) + _verdicts(m.render(3)) == [MUST_NOT, EITHER]
    m.set_samples_in_flight(1)
    assert _verdicts(m.render(2)) == [MUST_NOT, MUST]
    m.set_param("fuse", 0)                                        # any other tunable: eligibility is no longer known
    assert _verdicts(m.render(2)) == [MUST_NOT, EITHER]
    m.set_param("path_kernel", 1)                                 # a one-launch PATH batch leaves an earlier batch's stage alone:
    m.set_samples_in_flight(2)
    assert _verdicts(m.render(3)) + _verdicts(m.render(2)) == [MUST_NOT, EITHER, EITHER]    # 2 + 1, then 2 (after the 1)
    m.set_param("path_kernel", 0)
    assert _verdicts(m.render(3)) + _verdicts(m.render(2)) == [MUST_NOT, MUST_NOT, MUST_NOT]
    m.set_samples_in_flight(1)
    m.set_lens(True)
    assert _verdicts(m.render(2)) == [MUST_NOT, MUST_NOT] and not m.known
    copies = _model(S=3, scene=iseq.copies_scene(), kind="copies")
    assert _verdicts(copies.render(3)) + _verdicts(copies.render(3)) == [MUST_NOT, EITHER]


def test_the_campaign_holds_every_verdict():
    seen = {}
    for case in range(iseq.CAMPAIGN_CASES):
        head, ops = iseq.generate(iseq.CAMPAIGN_SEED, case)
        m, _ = iseq.replay(head, ops, oracle=False)
        for b in m.log:
            if not head["group"]:
                seen[b["verdict"]] = seen.get(b["verdict"], 0) + 1
    assert all(seen.get(v, 0) >= 30 for v in (MUST, MUST_NOT, EITHER)), seen
