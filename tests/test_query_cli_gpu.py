"""-m gpu: cuNVSMQuery (cunvsm_amd/host/query_main.cpp) end to end — from a checkpoint in the trainer's formats to TREC run files
and trec_eval-style means — against what this file computes with Model.set_param + Model.rank from the raw arrays and the mapping
dump that `query_tests --make-model` writes next to the checkpoint, and against tests/eval_reference.py.

Run lines are compared after parsing: topic, docno and rank exactly, the score as the float32 it prints (%.9g round-trips one).
Means are compared to the printed digits (four decimals: |printed - reference| <= 0.5e-4, plus 1e-9 for the decimal itself)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import eval_reference as er
from tests.conftest import ROOT
from tests.helpers import PARAMS, gpu_model
from tests.test_query_host import BIN as QUERY_TESTS, HOST_DIR, read_mapping_dump
from tests.test_trainer_gpu import CRANFIELD, run_trainer

pytestmark = pytest.mark.gpu

QUERY = os.path.join(ROOT, "cunvsm_amd", "bin", "cuNVSMQuery")
W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
VOCAB = ["term%d" % j for j in range(30)]
CUTOFFS = (5, 10, 20, 100, 1000)


def run_query(args, timeout=300):
    if not os.path.exists(QUERY):
        pytest.fail("%s is missing: __graft_entry__.build() builds it" % QUERY)
    return subprocess.run([QUERY] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


def tokens(text):
    return [t.lower() for t in re.findall(r"[A-Za-z0-9]+", text)]


class Corpus:
    """a 70-document collection, its stop list, the checkpoint of --make-model and a ranking-only handle loaded with its arrays"""

    def __init__(self, d):
        self.dir = d
        self.collection, self.stop = str(d / "docs.trectext"), str(d / "stop.txt")
        with open(self.collection, "w") as f:
            for i in range(1, 71):
                words = [VOCAB[(i * j + j * j) % 30] for j in range(1, 12)]
                f.write("<DOC>\n<DOCNO> DOC-%03d </DOCNO>\n<TEXT>\nThe %s of %s.\n</TEXT>\n</DOC>\n" % (i, " ".join(words[:6]), " ".join(words[6:])))
        with open(self.stop, "w") as f:
            f.write("the\nof\n")
        subprocess.check_call(["make", "-C", HOST_DIR, "build/query_tests"], stdout=subprocess.DEVNULL)
        self.base = str(d / "model")
        subprocess.check_call([QUERY_TESTS, "--make-model", self.collection, self.base, self.stop], stdout=subprocess.DEVNULL)
        self.checkpoint = self.base + "_3.hdf5"
        self.total_terms, self.terms, self.objects = read_mapping_dump(self.base + ".map.txt")
        self.docno_of = {m: docno for _, m, docno in self.objects}
        self.model_doc = {docno: m for _, m, docno in self.objects}
        self.outside = [w for w in VOCAB if w not in self.terms]                # in the index, not in the model (every 7th term)
        self.inside = [w for w in VOCAB if w in self.terms]
        assert len(self.objects) == 70 - 7 and len(self.outside) >= 3
        V, D = len(self.terms), len(self.objects)
        spec = dict(num_words=V, num_entities=D, word_dim=12, entity_dim=36, window=1, num_random=1, nonlinearity="tanh", update_method="sgd")
        self.model = gpu_model(spec, 8)
        for name, ext in ((W_NAME, "W"), (E_NAME, "E"), (T_NAME, "T"), (B_NAME, "b")):
            self.model.set_param(name, np.fromfile("%s.%s.f32" % (self.base, ext), np.float32))
        self.D = D
        a, b = self.inside, self.outside
        self.topics = {
            "topics_a": [("a1", "%s %s" % (a[0], a[5])),
                         ("a2", "%s, %s and zeppelin" % (a[1], b[0])),              # a word outside the model, one outside the index
                         ("a3", "The %s" % a[2]),                                   # a stopped word
                         ("a4", "%s zeppelin %s" % (b[1], b[2])),                   # nothing of it is in the model
                         ("a5", "%s %s %s" % (a[3], a[3], a[4])),                   # a word twice
                         ("a6", "%s; %s" % (a[6], a[7]))],                          # a ';' inside the text
            "topics_b": [("b1", a[8]), ("b2", "%s %s %s" % (a[9], a[10], a[11])), ("b3", "%s %s" % (a[12], a[0]))],
        }
        self.topic_paths = {}
        for name, topics in self.topics.items():
            self.topic_paths[name] = str(d / name)
            with open(self.topic_paths[name], "w") as f:
                f.write("".join("%s;%s\n" % t for t in topics) + "\n")
        # judged: documents of the model, documents the model lacks (every 9th) and docnos nobody knows; a3 has nothing relevant;
        # a4 is judged but never ranked; b3 is not judged at all
        def docs(*ids):
            return ["DOC-%03d" % i for i in ids]
        self.qrels = {
            "a1": list(zip(docs(1, 2, 3, 9, 10, 40) + ["NOPE-1"], [2, 0, 1, 1, 1, 3, 1])),
            "a2": list(zip(docs(5, 18, 50, 51, 52), [1, 2, 0, 0, 1])),
            "a3": list(zip(docs(7, 8), [0, 0])),
            "a4": list(zip(docs(1, 2), [1, 1])),
            "a5": list(zip(docs(60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70) + ["NOPE-2"], [1, 1, 1, 1, 2, 0, 1, 1, 1, 1, 3, 0])),
            "a6": list(zip(docs(27, 33), [1, 1])),
            "b1": list(zip(docs(11, 12, 13), [1, 0, 2])),
            "b2": list(zip(["NOPE-3"] + docs(35, 46), [2, 1, 1])),
        }
        self.qrel_path = str(d / "qrels")
        with open(self.qrel_path, "w") as f:
            for topic, judged in self.qrels.items():
                f.write("".join("%s 0 %s %d\n" % (topic, docno, g) for docno, g in judged))

    def expected(self, name, strict=False, self_information=False, linear=False, num_queries=None, top_k=1000, by_qrels=False):
        """[(topic, model term ids)] of the topics that are ranked, and Model.rank's result for them"""
        kept = []
        for topic, text in self.topics[name][:num_queries]:
            toks = tokens(text)
            terms = [self.terms[t][1] for t in toks if t in self.terms]
            if not terms or (strict and len(terms) < len(toks)):
                continue
            if by_qrels and topic not in self.qrels:
                continue
            kept.append((topic, terms))
        queries = [t for _, t in kept]
        weights = None
        if self_information:
            tf = {m: f for _, m, f in self.terms.values()}
            weights = [np.array([-np.log(tf[t] / self.total_terms) for t in terms], np.float64).astype(np.float32) for terms in queries]
        cands = None
        k = self.D if top_k == "all" else min(top_k, self.D)
        if by_qrels:
            cands = [[self.model_doc[d] for d, _ in self.qrels[topic] if d in self.model_doc] for topic, _ in kept]
            k = max(len(self.qrels[topic]) for topic, _ in kept)
        ids, scores, counts = self.model.rank(queries, top_k=k, weights=weights, candidates=cands, bias_coefficient=0.0,
                                              activation="identity" if linear else "tanh")
        return kept, ids, scores, counts

    def judged_ids(self, topic):
        return [(self.model_doc.get(docno, -1), g) for docno, g in self.qrels.get(topic, [])]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = Corpus(tmp_path_factory.mktemp("query_cli"))
    yield c
    c.model.close()


def read_run(path):
    rows = []
    with open(path) as f:
        for line in f:
            topic, q0, docno, rank, score, tag = line.split()
            assert q0 == "Q0" and tag == "cuNVSM"
            rows.append((topic, docno, int(rank), np.float32(score)))
    return rows


def expected_rows(corpus, kept, ids, scores, counts):
    rows = []
    for q, (topic, _) in enumerate(kept):
        rows += [(topic, corpus.docno_of[int(ids[q, r])], r + 1, scores[q, r]) for r in range(int(counts[q]))]
    return rows


def assert_same_run(got, want):
    assert [g[:3] for g in got] == [w[:3] for w in want]
    np.testing.assert_array_equal(np.array([g[3] for g in got], np.float32).view(np.uint32), np.array([w[3] for w in want], np.float32).view(np.uint32))


def base_args(corpus, out, *names):
    paths = [corpus.topic_paths[n] for n in names]
    return ["--index", corpus.collection, "--stopwords", corpus.stop, "--topics", paths[0]], paths[1:] + [corpus.checkpoint, out]


def printed_metrics(stdout):
    """[{metric: (topic, text)}] — one dict per topic file, in the order printed"""
    blocks, cur = [], None
    for line in stdout.splitlines():
        cols = line.split("\t")
        if len(cols) != 3:
            continue
        if cols[0] == "runid":
            cur = {}
            blocks.append(cur)
        if cols[1] == "all" and cur is not None:
            cur[cols[0]] = cols[2]
    return blocks


def test_two_topic_files_their_runs_and_the_printed_means(corpus, tmp_path):
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_a", "topics_b")
    r = run_query(flags + ["--qrels", corpus.qrel_path, "--per_query"] + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Skipping topic a4" in r.stderr
    blocks = printed_metrics(r.stdout)
    assert len(blocks) == 2
    for name, block in zip(("topics_a", "topics_b"), blocks):
        kept, ids, scores, counts = corpus.expected(name)
        assert [t for t, _ in kept] == [t for t, _ in corpus.topics[name] if t != "a4"]
        assert (counts == corpus.D).all()                                    # the default 1000, clipped to the model's documents
        assert_same_run(read_run("%s-%s" % (out, name)), expected_rows(corpus, kept, ids, scores, counts))
        ref = er.evaluate(ids, counts, [corpus.judged_ids(t) for t, _ in kept], CUTOFFS)
        evaluated = ref["num_rel"] > 0                                        # in the run, judged, something relevant: not a3, not b3
        assert [t for (t, _), e in zip(kept, evaluated) if not e] == (["a3"] if name == "topics_a" else ["b3"])
        assert block["num_q"] == str(int(evaluated.sum())) and block["topics"] == name
        for metric in er.names(CUTOFFS):
            if metric in er.INTEGER:
                assert block[metric] == str(int(ref[metric][evaluated].sum())), metric
            else:
                assert re.fullmatch(r"\d\.\d{4}", block[metric]), block[metric]
                assert abs(float(block[metric]) - ref[metric][evaluated].mean()) <= 0.5e-4 + 1e-9, metric
        for (t, _), e in zip(kept, evaluated):                                # --per_query: one line per metric and evaluated topic
            assert (("map\t%s\t" % t) in r.stdout) == bool(e)
        if name == "topics_a":                                                # -1 entries count: a1 holds two of them
            assert ref["num_rel"][0] == 6.0 and sum(d == -1 for d, _ in corpus.judged_ids("a1")) == 2
    # an existing run file is left alone, with a warning, and the other file is still written
    before = open(out + "-topics_a").read()
    os.remove(out + "-topics_b")
    r = run_query(flags + positional)
    assert r.returncode == 0 and "already exists" in r.stderr and "topics_a" in r.stderr
    assert open(out + "-topics_a").read() == before and os.path.exists(out + "-topics_b")


@pytest.mark.parametrize("case", ["strict", "self_information_linear", "num_queries_top_k_all", "top_k_5"])
def test_options(corpus, tmp_path, case):
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_a")
    extra, kwargs = {
        "strict": (["--strict"], dict(strict=True)),
        "self_information_linear": (["--self_information", "--linear", "--bias_coefficient", "0.5"], dict(self_information=True, linear=True)),
        "num_queries_top_k_all": (["--num_queries", "2", "--top_k", "all"], dict(num_queries=2, top_k="all")),
        "top_k_5": (["--top_k", "5"], dict(top_k=5)),
    }[case]
    r = run_query(flags + extra + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    kept, ids, scores, counts = corpus.expected("topics_a", **kwargs)
    assert [t for t, _ in kept] == {"strict": ["a1", "a5", "a6"], "self_information_linear": ["a1", "a2", "a3", "a5", "a6"],
                                    "num_queries_top_k_all": ["a1", "a2"], "top_k_5": ["a1", "a2", "a3", "a5", "a6"]}[case]
    assert_same_run(read_run(out + "-topics_a"), expected_rows(corpus, kept, ids, scores, counts))
    assert ("bias is never applied" in r.stderr) == (case == "self_information_linear")
    assert r.stdout == ""                                                     # no --qrels: nothing is evaluated


def test_top_k_from_qrels_ranks_the_judged_documents_only(corpus, tmp_path):
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_b")
    r = run_query(flags + ["--top_k", corpus.qrel_path, "--qrels", corpus.qrel_path] + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Skipping topic b3 as there are no judged documents." in r.stderr
    kept, ids, scores, counts = corpus.expected("topics_b", by_qrels=True)
    assert [t for t, _ in kept] == ["b1", "b2"] and list(counts) == [3, 2]   # NOPE-3 is nobody's document
    rows = read_run(out + "-topics_b")
    assert_same_run(rows, expected_rows(corpus, kept, ids, scores, counts))
    assert {d for t, d, _, _ in rows if t == "b2"} == {"DOC-035", "DOC-046"}
    block = printed_metrics(r.stdout)[0]
    ref = er.evaluate(ids, counts, [corpus.judged_ids(t) for t, _ in kept], CUTOFFS)
    assert block["num_q"] == "2" and block["num_rel_ret"] == str(int(ref["num_rel_ret"].sum())) == "4"
    assert abs(float(block["map"]) - ref["map"].mean()) <= 0.5e-4 + 1e-9


def test_a_batch_dump_finds_the_meta_file_of_its_run(corpus, tmp_path):
    shutil.copy(corpus.checkpoint, corpus.base + "_3_40.hdf5")
    out = str(tmp_path / "run")
    flags, _ = base_args(corpus, out, "topics_b")
    r = run_query(flags + [corpus.base + "_3_40.hdf5", out])
    assert r.returncode == 0, r.stderr[-3000:]
    assert_same_run(read_run(out + "-topics_b"), expected_rows(corpus, *corpus.expected("topics_b")))


def test_fatal_exits(corpus, tmp_path):
    broken = str(tmp_path / "broken")
    subprocess.check_call([QUERY_TESTS, "--make-model", corpus.collection, broken, corpus.stop, "word_entity_mapping-bias"], stdout=subprocess.DEVNULL)
    out = str(tmp_path / "run")
    flags, _ = base_args(corpus, out, "topics_b")
    r = run_query(flags + [broken + "_3.hdf5", out])
    assert r.returncode == 1 and "holds no dataset word_entity_mapping-bias" in r.stderr and not os.path.exists(out + "-topics_b")
    bad_topics = tmp_path / "bad_topics"
    bad_topics.write_text("1;fine\nno separator\n")
    r = run_query(["--index", corpus.collection, "--stopwords", corpus.stop, "--topics", str(bad_topics), corpus.checkpoint, out])
    assert r.returncode == 1 and "bad_topics:2" in r.stderr
    r = run_query(flags + ["--rerank_exact_matching_documents", corpus.checkpoint, out])
    assert r.returncode == 1 and "not offered" in r.stderr
    r = run_query(flags + ["--top_k", "nonsense", corpus.checkpoint, out])
    assert r.returncode == 1 and "--top_k" in r.stderr
    r = run_query(["--help"])
    assert r.returncode == 0 and "used at training time" in r.stdout and r.stdout.count("NOT OFFERED") == 3


def test_the_trainers_checkpoint_is_the_query_tools_input(tmp_path):
    """two epochs on Cranfield with the trainer, then the written checkpoint queried: names, shapes and mappings agree"""
    out = str(tmp_path / "lse")
    r = run_trainer(["--word_repr_size", "64", "--entity_repr_size", "64", "--window_size", "10", "--num_random_entities", "4", "--seed", "1",
                     "--update_method", "full_adam", "--nonlinearity", "tanh", "--batch_size", "1024", "--num_epochs", "2", "--output", out, CRANFIELD])
    assert r.returncode == 0, r.stderr[-3000:]
    topics = tmp_path / "topics"
    topics.write_text("1;boundary layer flow over a flat plate\n2;heat transfer in supersonic flow\n3;zzzzunknownzzzz\n")
    run = str(tmp_path / "run")
    q = run_query(["--index", CRANFIELD, "--topics", str(topics), "--top_k", "25", out + "_2.hdf5", run])
    assert q.returncode == 0, q.stderr[-3000:]
    rows = read_run(run + "-topics")
    for topic in ("1", "2"):
        mine = [r for r in rows if r[0] == topic]
        assert [r[2] for r in mine] == list(range(1, 26)) and len({r[1] for r in mine}) == 25
        assert (np.diff([r[3] for r in mine]) <= 0).all()
    assert len(rows) == 50 and "Skipping topic 3" in q.stderr
