"""Every retrieval entry point on ONE handle, in series order and then in reverse (tests/retrieval_rounds.py): infer, rank over all
documents and over candidate lists, evaluate, neighbors in word space without the query's own row and in projected-word space,
similarity in projected-word space, lexical_rank, rank_ensemble with judgments. The entry points share the handle's ranking scratch
and reuse some of its buffers with different meanings; every result must equal, bit for bit, the same call made as the only call of
a fresh handle with the same parameters. Three slabs, two rounds (NVSM_RANK_SLAB_MB=1)."""
import pytest

from tests import retrieval_rounds as rr
from tests.test_gpu_rank import same_bits

pytestmark = pytest.mark.gpu


def test_interleaved_calls_return_what_each_call_returns_alone(monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", rr.SLAB_MB)
    inp = rr.Inputs()
    calls = inp.calls()
    alone = {}
    for name, call in calls:              # the reference of each call: computed once, never changed
        m = inp.model()
        alone[name] = rr.arrays(call(m))
        m.close()
    m = inp.model()
    m.profile_enable(True)
    for name, call in calls + calls[::-1]:
        got = rr.arrays(call(m))
        assert [n for n, _ in got] == [n for n, _ in alone[name]], name
        for (what, x), (_, y) in zip(got, alone[name]):
            try:
                same_bits([x], [y])
            except AssertionError as e:
                raise AssertionError("%s %s differs from the call made alone: %s" % (name, what, e))
    names = set(m.profile())              # the series is what the docstring says: slabs with and without radix selection, every scan
    assert {"rank_select_radix", "rank_select_all", "rank_sort_lds", "rank_scan_candidates", "rank_eval", "lex_score", "fuse_lists",
            "nbr_scan", "nbr_project", "nbr_pairs", "rank_infer"} <= names, names
    m.close()
