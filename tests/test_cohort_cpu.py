"""A cohort registered to one template, without a GPU: the list files of tools/cohort_files.py, the reference-side cache of the level loop driven by
the oracle alone (with and without it: the same bits), and run_cohort's ordering and stop-on-error rule over a stub.  tests/test_gpu_cohort.py runs
the cohort over the MI355X path."""
import importlib.util
import os
import threading

import numpy as np
import pytest

import histmatch_literal as HL
import trans_excl_cases as C
from newmsm_amd import cohort, registration, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_tool():
    spec = importlib.util.spec_from_file_location("cohort_files", os.path.join(ROOT, "tools", "cohort_files.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- list files
def test_one_mesh_line_serves_every_subject():
    tool = load_tool()
    got = tool.subject_lists(["sunet.sphere"], ["a.func", "b.func", "c.func"])
    assert got == [("sunet.sphere", "a.func", None), ("sunet.sphere", "b.func", None), ("sunet.sphere", "c.func", None)]
    got = tool.subject_lists(["m0", "m1"], ["a", "b"], ["t0", "t1"])
    assert got == [("m0", "a", "t0"), ("m1", "b", "t1")]


def test_a_count_mismatch_names_both_counts():
    tool = load_tool()
    with pytest.raises(SystemExit, match="2 meshes, 3 data files"):
        tool.subject_lists(["m0", "m1"], ["a", "b", "c"])
    with pytest.raises(SystemExit, match=r"1 transformed meshes \(--trans\), 3 data files"):
        tool.subject_lists(["m0"], ["a", "b", "c"], ["t0"])


def test_out_of_scope_flags_are_refused_and_named_in_the_help(capsys):
    tool = load_tool()
    need = ["--meshes=m", "--data=d", "--refmesh=r", "--refdata=rd", "--out=o."]
    for flag in ("inweight", "refweight", "inanat", "refanat", "mask", "clusters"):
        with pytest.raises(SystemExit, match="--%s: .*out of scope" % flag):
            tool.main(need + ["--%s=x" % flag])  # refused before any file is opened
    with pytest.raises(SystemExit):
        tool.parse_args(["--help"])
    text = "".join(capsys.readouterr().out.split())  # (the help formatter breaks lines at blanks and hyphens)
    for phrase in ("cost-function weightings and aMSM surfaces per subject", "a weight mask for the statistics", "per-group statistics from a clustering file",
                   "a C++ executable twin", "sharing a target mesh or its direction table between contexts", "batching of the cost kernels across subjects"):
        assert "".join(phrase.split()) in text


# ---------------------------------------------------------------- the reference-side cache over the oracle
class MatchOps(HL.LiteralMatchMixin, C.MaskOracleOps):
    pass


def second_subject(case, seed):
    """another input data set against the same reference"""
    xyz, tri, _, ref, inside = case
    src = synthetic.features(synthetic.known_warp(xyz, seed=seed, rot_deg=2.0, amp=1.5), ref.shape[0], 31)
    src[:, inside & (ref[0] == 0.0)] = 0.0
    return xyz, tri, src, ref, inside


def assert_same_run(a, lab_a, b, lab_b):
    assert np.array_equal(a[0], b[0])
    assert len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert len(a[2]) == len(b[2]) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[2], b[2]))
    assert len(lab_a) == len(lab_b) > 0 and all(np.array_equal(x, y) for x, y in zip(lab_a, lab_b))


@pytest.mark.parametrize("variant", ["plain", "excl", "IN"])
def test_the_cache_changes_no_bit(variant):
    """run_multiresolution with and without ref_cache: np.array_equal results, for the subject that fills the cache and for another one that reads it"""
    kw = dict(plain={}, excl=dict(excl=True, cutthr=C.CUTTHR), IN=dict(intensity=True))[variant]
    make = (lambda: MatchOps(C.M.mcmc_optimise)) if variant == "IN" else C.oracle_ops
    case0 = C.pairwise_case(order=4, D=2, cap=variant == "excl")
    case1 = second_subject(case0, 77)
    assert not np.array_equal(case0[2], case1[2])
    levels = C.DISCRETE_PAIR
    cache = registration.ReferenceCache()
    for k, case in enumerate((case0, case1)):
        lab_c, lab_p = [], []
        cached = C.run(make(), case, levels, lab_c, ref_cache=cache, **kw)
        plain = C.run(make(), case, levels, lab_p, **kw)
        assert_same_run(cached, lab_c, plain, lab_p)
        assert cache.fills == len(levels) and cache.hits == k * len(levels)
    for entry in cache._entries.values():  # host arrays the cache owns
        f, m = entry[1]
        assert f.flags.owndata and not f.flags.writeable and (m is None) == (variant != "excl")
        assert m is None or (m.flags.owndata and not m.flags.writeable)


def test_a_run_that_differs_in_what_the_cache_depends_on_gets_its_own_entries():
    case = C.pairwise_case(order=4, D=1, cap=True)
    cache = registration.ReferenceCache()
    lab_a, lab_b, lab_p = [], [], []
    C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1], lab_a, ref_cache=cache)
    masked = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1], lab_b, ref_cache=cache, excl=True, cutthr=C.CUTTHR)
    plain = C.run(C.oracle_ops(), case, C.DISCRETE_PAIR[:1], lab_p, excl=True, cutthr=C.CUTTHR)
    assert cache.fills == 2 and cache.hits == 0
    assert_same_run(masked, lab_b, plain, lab_p)


# ---------------------------------------------------------------- run_cohort over a stub
class StubOps:
    made = []

    def __init__(self):
        self.thread = threading.get_ident()
        self.closed = False
        StubOps.made.append(self)

    def close(self):
        self.closed = True


@pytest.fixture
def stub(monkeypatch):
    """register_subject replaced by a function that does what the subject (a callable) says; records (subject, ops) in the order of the starts"""
    StubOps.made = []
    started = []

    def fake(ops, subject, ref_xyz, ref_tri, ref_data, levels, ref_cache=None, **run_kw):
        assert threading.get_ident() == ops.thread  # an ops object never leaves the thread that made it
        assert isinstance(ref_cache, registration.ReferenceCache)
        started.append((subject["id"], ops))
        return subject["do"](ops)

    monkeypatch.setattr(cohort, "register_subject", fake)
    return started


def run_stub(subjects, workers, **kw):
    return cohort.run_cohort(StubOps, subjects, None, None, None, [], workers=workers, **kw)


def test_results_come_back_in_subject_order(stub, monkeypatch):
    """two workers; subject 0 does not finish before subject 2 has: the order of completion is 1, 2, 0, the results are 0, 1, 2"""
    done = [threading.Event() for _ in range(3)]
    order = []

    def do(s, wait_for=None):
        def run(ops):
            if wait_for is not None:
                assert done[wait_for].wait(60)
            order.append(s)
            done[s].set()
            return dict(subject=s, env=os.environ.get("MSMHIP_HOST_THREADS"))
        return run

    subjects = [dict(id=0, do=do(0, wait_for=2)), dict(id=1, do=do(1)), dict(id=2, do=do(2))]
    monkeypatch.delenv("MSMHIP_HOST_THREADS", raising=False)
    res = run_stub(subjects, 2)
    assert [r["subject"] for r in res] == [0, 1, 2] and order == [1, 2, 0]
    assert len(StubOps.made) == 2 and all(o.closed for o in StubOps.made) and StubOps.made[0].thread != StubOps.made[1].thread
    assert all(r["env"] == "8" for r in res) and "MSMHIP_HOST_THREADS" not in os.environ  # 16 // 2 for the run, gone afterwards


def test_the_callers_thread_count_is_left_alone(stub, monkeypatch):
    monkeypatch.setenv("MSMHIP_HOST_THREADS", "3")
    res = run_stub([dict(id=s, do=lambda ops: os.environ["MSMHIP_HOST_THREADS"]) for s in range(3)], 4)
    assert res == ["3"] * 3 and os.environ["MSMHIP_HOST_THREADS"] == "3"
    assert len(StubOps.made) == 3  # at most one worker per subject


def test_a_failing_subject_stops_the_queue_one_worker(stub):
    def do(s):
        def run(ops):
            if s == 1:
                raise ValueError("subject one is broken")
            return s
        return run

    with pytest.raises(cohort.CohortError, match="subject 1 failed: ValueError: subject one is broken") as e:
        run_stub([dict(id=s, do=do(s)) for s in range(4)], 1)
    assert [s for s, _ in stub] == [0, 1] and e.value.subject == 1 and e.value.results == [0, None, None, None]
    assert isinstance(e.value.cause, ValueError) and all(o.closed for o in StubOps.made)


def test_a_failing_subject_stops_the_queue_two_workers(stub):
    """subject 0 is running when subject 1 fails: it finishes, its result is kept; the queue is not served to its end"""
    S = 40
    failed = threading.Event()

    def do(s):
        def run(ops):
            if s == 0:
                assert failed.wait(60)
            if s == 1:
                failed.set()
                raise RuntimeError("MSM_ERR_HIP (-2): stub")
            return s
        return run

    with pytest.raises(cohort.CohortError, match="subject 1 failed") as e:
        run_stub([dict(id=s, do=do(s)) for s in range(S)], 2)
    assert e.value.results[0] == 0 and e.value.results[1] is None
    assert len(stub) < S and e.value.results[-1] is None
    assert all(o.closed for o in StubOps.made)
