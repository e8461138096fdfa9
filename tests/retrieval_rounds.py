"""One fixed series of retrieval calls on one small collection, shared by tests/test_gpu_retrieval_rounds.py (every call's result on
a handle that has made all the others equals, bit for bit, the call made alone on a fresh handle) and tools/rank_trace.py (the same
series under a tracer, for comparing two builds of the library).

The collection is the 9001-document, 300-query case of tests/lexical_reference.py on the model of tests/test_gpu_lexical.py
(dimensions 8); with NVSM_RANK_SLAB_MB=1 a round of 256 queries sees the documents as three slabs of 4096 rows (the last one 809),
and 300 queries are two rounds. The entry points share Model::RankScratch, several of whose buffers change their meaning from call
to call (ids, offsets, self): a call must not depend on what the call before it left there."""
import numpy as np

from tests import lexical_reference as lr

DOCUMENTS, QUERIES = 9001, 300
SLAB_MB = "1"                              # NVSM_RANK_SLAB_MB, read when a handle is created


class Inputs:
    def __init__(self):
        self.tokens, self.offsets, self.queries = lr.case_inputs(DOCUMENTS, QUERIES)
        rs = np.random.RandomState(19)
        # candidate lists: none, one, duplicates in any order, up to 600 documents
        self.candidates = [list(rs.randint(0, DOCUMENTS, rs.randint(0, 3) * rs.randint(0, 300))) for _ in range(QUERIES)]
        self.candidates[3] = [7, 7, 5, 7]
        self.judgments = [[(int(d), int(rs.randint(0, 3))) for d in rs.choice(DOCUMENTS, rs.randint(0, 40), replace=False)] for _ in range(QUERIES)]
        self.words = rs.choice(lr.NUM_WORDS, QUERIES, replace=False)             # 300 query rows: two rounds
        self.pairs = rs.randint(0, lr.NUM_WORDS, (2, 2500))                       # 2500 pairs: two rounds of nvsm_similarity

    def model(self):
        """a fresh handle with the parameters every handle of this collection gets, and the corpus uploaded"""
        from tests.test_gpu_lexical import lexical_model
        return lexical_model(DOCUMENTS, corpus=(self.tokens, self.offsets))

    def calls(self):
        """(name, call) in series order; a call takes the handle and returns arrays (or a dict of arrays in front of them)"""
        x = self
        return [
            ("infer", lambda m: (m.infer(x.queries),)),
            ("rank", lambda m: m.rank(x.queries, top_k=1000)),                   # the last slab has fewer rows than top_k
            ("rank_candidates", lambda m: m.rank(x.queries, top_k=5, candidates=x.candidates)),
            ("evaluate", lambda m: m.evaluate(x.queries, x.judgments, top_k=10, cutoffs=(5, 10), return_ranking=True)),
            ("neighbors_words", lambda m: m.neighbors("words", ids=x.words, top_k=7, exclude_self=True)),
            ("neighbors_projected", lambda m: m.neighbors("projected_words", ids=x.words, top_k=7, similarity="dot")),
            ("similarity_projected", lambda m: (m.similarity("projected_words", x.pairs[0], x.pairs[1]),)),
            ("lexical_rank", lambda m: m.lexical_rank(x.queries, top_k=10)),
            ("rank_ensemble", lambda m: m.rank_ensemble(x.queries, judgments=x.judgments, top_k=10, cutoffs=(5, 10))),
        ]


def arrays(result):
    """a call's result as a flat list of (name, array)"""
    out = []
    for i, part in enumerate(result):
        if isinstance(part, dict):
            out += [(name, part[name]) for name in sorted(part)]
        else:
            out.append(("[%d]" % i, part))
    return out
