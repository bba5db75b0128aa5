"""Batch queries from an intropolis file on the GPU: the rows morna_build_query_rows makes, the approximate and exact
answers of MornaSearch.search_nn_batch / exact_search_nn_batch, the index left as it was, row shards in one process and
`morna search --intropolis / --query-ids`.  -m gpu"""
import contextlib
import io
import re

import numpy as np
import pytest

from test_query_batch_cpu import finalize_rows, query_terms

pytestmark = pytest.mark.gpu

N_INDEX, N_QUERY, J, THRESHOLD, TREES = 3000, 300, 12000, 30, 10
ZERO_SAMPLE = 99999999      # a query sample whose only junction is outside the vocabulary


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    from morna_amd.synth import index_and_query_files
    d = tmp_path_factory.mktemp("cohort")
    ipath, qpath = str(d / "index.tsv.gz"), str(d / "queries.tsv")
    ids = index_and_query_files(ipath, qpath, N_INDEX, N_QUERY, J=J)
    with open(qpath, "a") as fh:
        fh.write("chrZ\t1\t2\t+\tGT\tAG\t%d\t5\n" % ZERO_SAMPLE)
    meta = str(d / "meta.txt")
    with open(meta, "w") as fh:
        for s in ids["index_ids"].tolist():
            fh.write("%d tissue_%d sex_%d\n" % (s, s % 7, s % 2))
    return dict(dir=d, index=ipath, queries=qpath, ids=ids, meta=meta, bases={})


def index_base(cohort, dim, shards=1):
    """The index of the cohort's index file at `dim` (built once per module)."""
    key = (dim, shards)
    if key not in cohort["bases"]:
        from morna_amd.index import go_index
        base = str(cohort["dir"] / ("idx_%d_%d" % (dim, shards)))
        go_index(cohort["index"], base, dim, TREES, None, THRESHOLD, 1024, False, cohort["meta"], native=True, shards=shards)
        cohort["bases"][key] = base
    return cohort["bases"][key]


def reference_rows(searcher, path):
    """update_query over every sample's lines + finalize_query, in Python, in first-appearance order of the samples."""
    T = query_terms(path, dict(searcher.sample_frequencies), searcher.sample_count)
    ext = T.arrays()["ext_ids"].tolist()
    rows, _ = finalize_rows(path, dict(searcher.sample_frequencies), searcher.sample_count, searcher.dim, ext)
    return ext, rows


@pytest.mark.parametrize("dim", [3000, 257, 12000])
def test_rows_equal_finalize_query(cohort, dim):
    from morna_amd.search import MornaSearch
    from oracle import capi
    s = MornaSearch(index_base(cohort, dim))
    batch = s.queries_from_intropolis(cohort["queries"])
    ext, want = reference_rows(s, cohort["queries"])
    assert batch.ext_ids == ext and batch.n == N_QUERY + 1
    assert ext[-1] == ZERO_SAMPLE
    r64, r32 = s.annoy_index.get_query_rows()
    assert r64.tobytes() == want.tobytes()
    assert r32.tobytes() == want.astype(np.float32).tobytes()
    assert not r64[-1].any() and r64[:-1].any()
    capi.build()
    keys_of = {}
    from morna_amd.index import tokenize_line
    with open(cohort["queries"]) as fh:
        for line in fh:
            key, samples, covs = tokenize_line(line)
            if key in s.sample_frequencies:
                for smp, c in zip(samples, covs):
                    keys_of.setdefault(smp, {}).setdefault(key, 0)
                    keys_of[smp][key] += c
    for q in (0, 1, 17, N_QUERY - 1):
        kk = keys_of[ext[q]]
        o = capi.finalize_query(list(kk), list(kk.values()), [s.sample_frequencies[k] for k in kk], s.sample_count, dim)
        assert o.tobytes() == r64[q].tobytes()


@pytest.mark.parametrize("dim", [3000, 257])
def test_index_input_as_queries_gives_its_rows(cohort, dim):
    """The index's own input (no duplicate keys, no sample twice in a line) as the query file: float32(rows) are the
    index's rows, matched by external id; samples seen only on lines below the threshold get a zero row."""
    from morna_amd.search import MornaSearch
    s = MornaSearch(index_base(cohort, dim))
    batch = s.queries_from_intropolis(cohort["index"])
    r64, r32 = s.annoy_index.get_query_rows()
    X = s.annoy_index.get_items()
    assert r32.tobytes() == r64.astype(np.float32).tobytes()
    n_zero = 0
    for q, ext in enumerate(batch.ext_ids):
        if ext in s.internal_id_map:
            assert r32[q].tobytes() == X[s.internal_id_map[ext]].tobytes(), ext
        else:
            assert not r64[q].any()
            n_zero += 1
    assert len(batch.ext_ids) - n_zero == X.shape[0]


@pytest.mark.parametrize("dim", [3000, 257, 12000])
def test_approximate_batch_equals_host_queries(cohort, dim):
    from morna_amd.search import MornaSearch
    s = MornaSearch(index_base(cohort, dim))
    batch = s.queries_from_intropolis(cohort["queries"])
    r64, r32 = s.annoy_index.get_query_rows()
    for k in (1, 20, 100):
        for search_k in (-1, 100):
            got = s.search_nn_batch(batch, k, search_k, include_distances=True)
            ids, d, cnt = s.annoy_index.get_nns_by_vector_batch(r32, k, search_k)
            assert len(got) == batch.n
            for q in range(batch.n):
                m = int(cnt[q])
                assert got[q][0] == ids[q, :m].tolist(), (k, search_k, q)
                assert np.array(got[q][1], np.float32).tobytes() == d[q, :m].tobytes()
    plain = s.search_nn_batch(batch, 20, 100, include_distances=False)
    assert all(len(r) == 1 for r in plain)
    for q in (0, 5, 77, batch.n - 1):                       # one query at a time, as `search -f raw` does it
        s.query_sample = [float(x) for x in r64[q]]
        assert s.search_nn(20, 100, include_distances=True) == s.search_nn_batch(batch, 20, 100)[q]


@pytest.mark.parametrize("dim", [3000, 257, 12000])
def test_exact_batch_equals_host_queries(cohort, dim):
    from morna_amd.search import MornaSearch
    s = MornaSearch(index_base(cohort, dim))
    batch = s.queries_from_intropolis(cohort["queries"])
    r64, _ = s.annoy_index.get_query_rows()
    for k in (1, 20):
        got = s.exact_search_nn_batch(batch, k, include_distances=True)
        ids, d, cnt = s.annoy_index.exact_search_batch(r64, k)
        for q in range(batch.n):
            m = int(cnt[q])
            assert m >= 0 and not isinstance(got[q], Exception)
            assert got[q][0] == ids[q, :m].tolist(), (k, q)
            assert np.array(got[q][1], np.float64).tobytes() == d[q, :m].tobytes()
    for q in (0, 3, batch.n - 1):                           # the zero row included
        s.query_sample = [float(x) for x in r64[q]]
        assert s.exact_search_nn(20) == s.exact_search_nn_batch(batch, 20)[q]
    if dim == 257:
        from oracle import capi
        capi.build()
        X = s.annoy_index.get_items()
        got = s.exact_search_nn_batch(batch, 10)
        for q in list(range(0, batch.n, 37)) + [batch.n - 1]:
            rid, rd = capi.exact_search(X, r64[q], 10)
            assert got[q][0] == rid.tolist() and np.array(got[q][1]).tobytes() == rd.tobytes(), q


def test_index_untouched_and_second_batch_replaces_first(cohort):
    from morna_amd.search import MornaSearch
    s = MornaSearch(index_base(cohort, 3000))
    a = s.annoy_index
    items = np.arange(0, 200, 7, dtype=np.int32)

    def state():
        f = a.get_forest()
        return (a.get_items().tobytes(), a.get_norms2().tobytes(), [v.tobytes() for v in f.values()],
                [x.tobytes() for x in a.get_nns_by_item_batch(items, 20, 100)],
                [x.tobytes() for x in a.exact_search_by_item_batch(items, 20)])
    before = state()
    first = s.queries_from_intropolis(cohort["queries"])
    r_first = a.get_query_rows()[0]
    s.search_nn_batch(first, 20, 100)
    s.exact_search_nn_batch(first, 20)
    assert state() == before
    second = s.queries_from_intropolis(cohort["index"])
    assert state() == before
    r_second = a.get_query_rows()[0]
    assert r_second.shape[0] == second.n != first.n
    _, want = reference_rows(s, cohort["index"])
    assert r_second.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="replaced"):
        s.search_nn_batch(first, 20, 100)
    third = s.queries_from_intropolis(cohort["queries"])
    assert a.get_query_rows()[0].tobytes() == r_first.tobytes()
    assert s.exact_search_nn_batch(third, 5) == s.exact_search_nn_batch(third, 5)


def test_local_shards(cohort):
    from morna_amd.search import MornaSearch
    from morna_amd.shards import LocalShards
    s = MornaSearch(index_base(cohort, 3000, shards=2))
    assert isinstance(s.annoy_index, LocalShards)
    whole = MornaSearch(index_base(cohort, 3000))
    batch = s.queries_from_intropolis(cohort["queries"])
    wbatch = whole.queries_from_intropolis(cohort["queries"])
    r64, r32 = whole.annoy_index.get_query_rows()
    assert batch.rows64.tobytes() == r64.tobytes() and batch.rows32.tobytes() == r32.tobytes()
    ids, d, cnt = s.annoy_index.get_nns_by_vector_batch(r32, 20, 100)
    got = s.search_nn_batch(batch, 20, 100)
    for q in range(batch.n):
        assert got[q][0] == ids[q, :int(cnt[q])].tolist()
        assert np.array(got[q][1], np.float32).tobytes() == d[q, :int(cnt[q])].tobytes()
    ids, d, cnt = s.annoy_index.exact_search_batch(r64, 20)
    got = s.exact_search_nn_batch(batch, 20)
    want = whole.exact_search_nn_batch(wbatch, 20)
    for q in range(batch.n):
        assert got[q][0] == ids[q, :int(cnt[q])].tolist()
        assert np.array(got[q][1]).tobytes() == d[q, :int(cnt[q])].tobytes()
        assert got[q][0] == want[q][0] and np.array(got[q][1]).tobytes() == np.array(want[q][1]).tobytes()


def _blocks(text):
    parts = re.split(r"^# query (-?\d+)\n", text, flags=re.M)
    assert parts[0] == ""
    return [(int(parts[i]), parts[i + 1]) for i in range(1, len(parts), 2)]


def _raw_stream(path, sample):
    out = []
    with open(path) as fh:
        for line in fh:
            t = line.rstrip("\n").split("\t")
            for smp, c in zip(t[-2].split(","), t[-1].split(",")):
                if int(smp) == sample:
                    out.append("%s\t%s\t%s\t%s\n" % (t[0], t[1], t[2], c))
    return "".join(out)


@pytest.mark.parametrize("flags", [["-d"], ["-d", "-m"], ["-e", "-d"]])
def test_cli_intropolis_blocks_equal_raw_runs(cohort, flags):
    from morna_amd import cli
    base = index_base(cohort, 3000)
    out = io.StringIO()
    assert cli.main(["search", "-x", base, "--intropolis", cohort["queries"], "-f", "bed"] + flags, stdout=out) == 0
    blocks = _blocks(out.getvalue())
    assert len(blocks) == N_QUERY + 1
    for sample, body in blocks[:6] + blocks[-2:]:
        one = io.StringIO()
        assert cli.main(["search", "-x", base, "-f", "raw"] + flags, stdin=io.StringIO(_raw_stream(cohort["queries"], sample)),
                        stdout=one) == 0
        assert body == one.getvalue(), sample


@pytest.mark.parametrize("flags", [["-d"], ["-d", "-m"], []])
def test_cli_query_ids_blocks_equal_q_runs(cohort, flags):
    from morna_amd import cli
    from morna_amd.search import MornaSearch
    base = index_base(cohort, 3000)
    indexed = sorted(MornaSearch(base).internal_id_map)
    picks = [indexed[0], indexed[10], indexed[500], indexed[-1]]
    out = io.StringIO()
    assert cli.main(["search", "-x", base, "--query-ids", ",".join(map(str, picks))] + flags, stdout=out) == 0
    blocks = _blocks(out.getvalue())
    assert [b[0] for b in blocks] == picks
    for sample, body in blocks:
        one = io.StringIO()
        with contextlib.redirect_stdout(one):
            assert cli.main(["search", "-x", base, "-q", str(sample)] + flags, stdout=one) == 0
        assert body == one.getvalue(), sample
    out = io.StringIO()
    unknown = cohort["ids"]["query_ids"][0]
    with pytest.raises(ValueError, match="Querying sample id %d is not possible" % unknown):
        cli.main(["search", "-x", base, "--query-ids", "%d,%d" % (picks[0], unknown)], stdout=out)
    assert out.getvalue() == ""
