"""JunctionStore.explain on the GPU (csrc/explain.hip): every sum as its 8 bytes, every count and every
entry of the top lists against the plain-Python restatement of the contract in explain_ref.py.  Stores come from
JunctionStore.from_arrays.  -m gpu"""
import numpy as np
import pytest

from explain_ref import assert_pair, bits, explain_pair
from test_gpu_unhashed import array_store, random_rows

pytestmark = pytest.mark.gpu


def check_lists(got, queries, lists, rows_by_ext, w, top, what=""):
    """got: what explain returned for `queries` ((lines, cov) pairs) and `lists` (external ids in rank order)."""
    assert len(got) == len(queries) and [len(g) for g in got] == [len(lst) for lst in lists]
    for q, (ql, qc) in enumerate(queries):
        for rank, ext in enumerate(lists[q]):
            rl, rc = rows_by_ext[int(ext)]
            assert_pair(got[q][rank], explain_pair(ql, qc, rl, rc, w, top), "%s query %d rank %d" % (what, q, rank))


def hot_rows(rng, lengths, hot, zero_share=0.05):
    """Rows on the lines `hot` (so that rows and queries meet), a share of their coverages 0."""
    rows = []
    for n in lengths:
        l = np.sort(rng.choice(hot, size=n, replace=False)).astype(np.int32)
        c = np.ceil(rng.lognormal(1.0, 1.5, size=n)).astype(np.int32)
        c[rng.random(n) < zero_share] = 0
        rows.append((l, c))
    return rows


@pytest.mark.parametrize("n_lines,qt", [(5000, 16), (40000, 8)])
def test_row_and_query_lengths(n_lines, qt):
    """The chunk edges of a wave and a row of many chunks, against queries short and long, either side of the QT rule."""
    rng = np.random.default_rng(n_lines)
    hot = rng.choice(n_lines, size=4500, replace=False)
    w = np.where(rng.random(n_lines) < 0.2, 0.0, rng.uniform(0.05, 6.0, n_lines))
    rows = hot_rows(rng, [0, 1, 63, 64, 65, 128, 200, 4100], hot)
    queries = hot_rows(rng, [0, 1, 64, 3000], hot)
    store, ext = array_store(rows, n_lines, w)
    by_ext = {int(e): rows[i] for i, e in enumerate(ext)}
    lists = [list(ext)] * len(queries)
    for top in (10, 64):
        got = store.explain(queries, lists, top)
        check_lists(got, queries, lists, by_ext, w, top, "top %d" % top)
    stats = store.explain_stats()
    assert stats["queries_per_pass"] == qt and stats["passes"] == 1 and stats["pairs"] == 32 and stats["kernel_ms"] > 0
    assert stats["entries"] == 4 * sum(len(l) for l, _ in rows) and stats["bytes"] == 8 * stats["entries"]
    assert max(p.shared for g in got for p in g) > 64 and min(p.shared for g in got for p in g) == 0
    # the store's own rows as the queries: every row against every row
    got = store.explain_by_sample(ext, [list(ext)] * len(ext), 7)
    check_lists(got, rows, [list(ext)] * len(ext), by_ext, w, 7, "by sample")


def test_intersections():
    """None, all, exactly one line, and shared lines in the row's last partial chunk only."""
    rng = np.random.default_rng(3)
    n_lines = 1000
    w = rng.uniform(0.05, 6.0, n_lines)
    row = (np.arange(0, 400, 2, dtype=np.int32), rng.integers(1, 50, 200).astype(np.int32))       # 200 entries: 3 chunks and 8
    store, ext = array_store([row], n_lines, w)
    cov = lambda n: rng.integers(1, 50, n).astype(np.int32)
    queries = [(np.arange(1, 400, 2, dtype=np.int32), cov(200)),                 # none
               (row[0].copy(), cov(200)),                                      # all
               (np.array([77, 138, 501], np.int32), cov(3)),                   # exactly one: line 138
               (np.sort(np.concatenate([row[0][192:], np.arange(1, 99, 2)])).astype(np.int32), cov(8 + 49))]
    lists = [[ext[0]]] * 4
    got = store.explain(queries, lists, 10)
    check_lists(got, queries, lists, {int(ext[0]): row}, w, 10)
    assert [g[0].shared for g in got] == [0, 200, 1, 8]
    assert got[0][0].distance == np.sqrt(2.0) and len(got[0][0].lines) == 0 and got[0][0].qq_shared == 0.0
    assert got[1][0].pp_shared == got[1][0].pp and got[1][0].qq_shared == got[1][0].qq
    assert got[2][0].lines.tolist() == [138] and got[2][0].n_q == 3
    assert got[3][0].lines.min() >= row[0][192]


def test_lines_of_weight_zero_and_coverage_zero():
    """`shared` is defined on values: a line of weight 0, or an entry of coverage 0, is not shared, wherever it stands."""
    n_lines = 600
    w = np.full(n_lines, 1.5)
    w[100:200] = 0.0        # weight 0, on the query side only
    w[200:300] = 0.0        # ... on the result side only
    w[300:400] = 0.0        # ... on both
    row_l = np.concatenate([np.arange(0, 100), np.arange(200, 400), np.arange(400, 500)]).astype(np.int32)
    q_l = np.concatenate([np.arange(0, 200), np.arange(300, 450)]).astype(np.int32)
    row_c = np.full(len(row_l), 3, np.int32)
    q_c = np.full(len(q_l), 2, np.int32)
    row_c[10:20] = 0         # coverage 0 in the row on lines the query holds
    q_c[30:40] = 0           # ... in the query on lines the row holds
    row_c[50] = q_c[50] = 0  # ... in both
    store, ext = array_store([(row_l, row_c)], n_lines, w)
    got = store.explain([(q_l, q_c)], [[ext[0]]], 64)
    want = explain_pair(q_l, q_c, row_l, row_c, w, 64)
    assert_pair(got[0][0], want)
    # shared: lines 0..99 and 400..449, without the 21 entries of coverage 0 on one side or both
    assert got[0][0].shared == 100 + 50 - 21
    assert got[0][0].n_r == 200 - 11 and got[0][0].n_q == 100 + 50 - 11
    assert got[0][0].lines.tolist() == [l for l in range(0, 100) if not (10 <= l < 20 or 30 <= l < 40 or l == 50)][:64]


def test_ties_are_ordered_by_line():
    """Weights that are powers of two and small integer coverages: the products are exact and many terms are equal."""
    n_lines = 2000
    w = np.where(np.arange(n_lines) % 3 == 0, 0.5, 2.0)
    w[np.arange(n_lines) % 3 == 1] = 4.0

    def run(row_l, row_c, q_l, q_c, top):
        store, ext = array_store([(np.asarray(row_l, np.int32), np.asarray(row_c, np.int32))], n_lines, w)
        got = store.explain([(np.asarray(q_l, np.int32), np.asarray(q_c, np.int32))], [[ext[0]]], top)[0][0]
        assert_pair(got, explain_pair(q_l, q_c, row_l, row_c, w, top))
        return got

    same = np.arange(0, 1800, 3)                                             # 600 lines of weight 0.5
    row_l = same[:300]
    shared_l = same[100:300]                                                  # 200 shared lines, equal terms
    got = run(row_l, [4] * 300, shared_l, [2] * 200, 5)
    assert got.shared == 200 and got.lines.tolist() == shared_l[:5].tolist() and set(got.terms.tolist()) == {2.0}
    # the largest term in the last lane of the last chunk
    c = [3] * 128
    c[-1] = 9
    got = run(same[:128], c, same[:128], [1] * 128, 5)
    assert got.lines.tolist() == [int(same[127])] + same[:4].tolist()
    # ascending terms: every entry is inserted; descending: none after the first chunk
    up = list(range(1, 201))
    got = run(same[:200], up, same[:200], [2] * 200, 64)
    assert got.lines.tolist() == same[:200][::-1][:64].tolist()
    got = run(same[:200], up[::-1], same[:200], [2] * 200, 64)
    assert got.lines.tolist() == same[:64].tolist()
    # pairs of equal terms among ascending ones, on mixed weights
    lines = np.arange(0, 390)
    got = run(lines, [1 + (i // 2) % 7 for i in range(390)], lines, [1 + (i // 5) % 3 for i in range(390)], 20)
    assert len(set(got.terms.tolist())) < 20


@pytest.mark.parametrize("top", [1, 5, 64])
def test_top_and_the_sum_of_a_whole_list(top):
    rng = np.random.default_rng(5)
    n_lines = 900
    w = rng.uniform(0.05, 6.0, n_lines)
    rows = random_rows(rng, [3, 40, 64, 70, 300], n_lines)
    store, ext = array_store(rows, n_lines, w)
    by_ext = {int(e): rows[i] for i, e in enumerate(ext)}
    queries = random_rows(rng, [200, 500], n_lines)
    lists = [list(ext)] * 2
    got = store.explain(queries, lists, top)
    check_lists(got, queries, lists, by_ext, w, top)
    whole = 0
    for g in got:
        for p in g:
            assert len(p.lines) == min(top, p.shared)
            if top >= p.shared:                                              # top larger than shared: the whole intersection
                acc = 0.0
                for _, term in sorted(zip(p.lines.tolist(), p.terms.tolist())):
                    acc = acc + term
                assert bits(acc) == bits(p.pq)
                whole += 1
    assert whole >= (1 if top == 1 else 2 if top == 5 else 6)


@pytest.fixture(scope="module")
def sixty():
    rng = np.random.default_rng(17)
    n_lines = 3000
    w = np.where(rng.random(n_lines) < 0.15, 0.0, rng.uniform(0.05, 6.0, n_lines))
    rows = random_rows(rng, [int(x) for x in rng.integers(0, 320, 60)], n_lines)
    store, ext = array_store(rows, n_lines, w)
    return dict(store=store, ext=ext, rows=rows, w=w, by_ext={int(e): rows[i] for i, e in enumerate(ext)}, n_lines=n_lines)


@pytest.mark.parametrize("k", [1, 20, 64])
def test_batching(sixty, k):
    """One tile, one more than a tile, several; ragged lists, an empty one, an id at two ranks, a query among its results."""
    store, ext, rows, w = sixty["store"], sixty["ext"], sixty["rows"], sixty["w"]
    rng = np.random.default_rng(k)
    for nq in (1, 16, 17, 40):
        q_ids = [int(ext[(3 * q + k) % 60]) for q in range(nq)]
        lists = []
        for q in range(nq):
            n = k if q % 4 == 0 else int(rng.integers(0, k + 1))
            lst = [int(x) for x in rng.choice(ext, size=n, replace=True)]
            if n >= 2:
                lst[-1] = lst[0]                                             # an id at two ranks
            if n >= 1 and q % 3 == 0:
                lst[n // 2] = q_ids[q]                                       # the query among its own results
            lists.append(lst)
        if nq > 2:
            lists[2] = []
        if nq == 1:
            lists[0] = ([q_ids[0]] * k)[:k]
        got = store.explain_by_sample(q_ids, lists, 6)
        check_lists(got, [sixty["by_ext"][s] for s in q_ids], lists, sixty["by_ext"], w, 6, "nq %d k %d" % (nq, k))
        stats = store.explain_stats()
        assert stats["queries_per_pass"] == 16 and stats["passes"] == -(-nq // 16)
        assert stats["pairs"] == sum(len(lst) for lst in lists)
        for q in range(nq):
            for rank, s in enumerate(lists[q]):
                if s == q_ids[q] and got[q][rank].pp > 0:
                    assert got[q][rank].distance < 1e-7 and got[q][rank].pp == got[q][rank].qq == got[q][rank].pq
                if rank and s == lists[q][0]:
                    assert got[q][rank].sums.tobytes() == got[q][0].sums.tobytes()


def test_identities_against_the_unhashed_search():
    """For every pair of a 300-sample store: the distance nearest_by_sample returns with the results as its population, and
    the pp of row_norms."""
    rng = np.random.default_rng(23)
    n_lines, n = 2500, 300
    w = np.where(rng.random(n_lines) < 0.1, 0.0, rng.uniform(0.05, 6.0, n_lines))
    rows = random_rows(rng, [int(x) for x in rng.integers(1, 200, n)], n_lines)
    store, ext = array_store(rows, n_lines, w)
    ids, d, cnt = store.nearest_by_sample(ext, ext, n)
    assert (cnt == n).all()
    by_position = np.zeros((n, n), np.float64)
    np.put_along_axis(by_position, ids.astype(np.int64), d, axis=1)
    norms = store.row_norms(ext)
    got = store.explain_by_sample(ext, [list(ext)] * n, 1)
    assert store.explain_stats()["pairs"] == n * n
    dist = np.array([[p.distance for p in g] for g in got])
    pp = np.array([[p.pp for p in g] for g in got])
    qq = np.array([[p.qq for p in g] for g in got])
    assert dist.tobytes() == by_position.tobytes()
    assert pp.tobytes() == np.tile(norms, (n, 1)).tobytes()
    assert qq.tobytes() == np.repeat(norms, n).reshape(n, n).tobytes()
    for q in (0, 150, 299):
        for r in (0, 7, 299):
            assert_pair(got[q][r], explain_pair(*rows[q], *rows[r], w, 1))


def as_bytes(got):
    return b"".join(p.sums.tobytes() + p.counts.tobytes() + p.lines.tobytes() + p.terms.tobytes() + p.cov_r.tobytes()
                    for g in got for p in g)


def test_deterministic_and_independent_of_qt(sixty, monkeypatch):
    store, ext = sixty["store"], sixty["ext"]
    q_ids = [int(x) for x in ext[:37]]
    lists = [[int(ext[(q + 5 * r) % 60]) for r in range(12)] for q in range(37)]
    first = as_bytes(store.explain_by_sample(q_ids, lists, 10))
    assert as_bytes(store.explain_by_sample(q_ids, lists, 10)) == first
    for qt in (4, 8, 16):
        monkeypatch.setenv("MORNA_UNHASHED_QT", str(qt))
        assert as_bytes(store.explain_by_sample(q_ids, lists, 10)) == first
        stats = store.explain_stats()
        assert stats["queries_per_pass"] == qt and stats["passes"] == -(-37 // qt)


def test_errors(sixty):
    from morna_amd.junctions import JunctionStore
    store, ext, rows = sixty["store"], sixty["ext"], sixty["rows"]
    a, b = int(ext[0]), int(ext[1])
    with pytest.raises(IndexError) as e:
        store.explain_by_sample([a], [[b, 424242]], 5)
    assert "424242" in str(e.value)
    assert store.explain_stats()["pairs"] == 0                                # a refused call leaves no statistics
    with pytest.raises(IndexError) as e:
        store.explain_by_sample([a, 515151], [[b], [b]], 5)
    assert "515151" in str(e.value)
    for top in (0, 65):
        with pytest.raises(ValueError) as e:
            store.explain_by_sample([a], [[b]], top)
        assert "64" in str(e.value)
    with pytest.raises(ValueError) as e:
        store.explain_by_sample([a], [[b] * 1025], 5)
    assert "1024" in str(e.value)
    import ctypes as C
    from morna_amd._lib import lib, ptr
    q, res, n_res, out = np.array([a], np.int64), np.array([b], np.int64), np.array([0], np.int32), C.c_void_p()
    for k in (0, 1025):
        assert lib().morna_jstore_explain_by_sample(store._p, ptr(q), 1, ptr(res), ptr(n_res), k, 5, C.byref(out)) == -1
        assert b"1024" in lib().morna_last_error() and not out.value
    with pytest.raises(ValueError) as e:
        store.explain([([1, 5], [2, -1])], [[b]], 5)
    assert "line 5" in str(e.value)
    with pytest.raises(ValueError):
        store.explain([([5, 1], [2, 1])], [[b]], 5)                          # lines that do not ascend
    # a negative coverage in a result row, and in a query row
    bad = [(l.copy(), c.copy()) for l, c in rows[:6]]
    at = max(range(6), key=lambda i: len(bad[i][0]))
    bad[at][1][len(bad[at][1]) // 2] = -3
    neg, nxt = array_store(bad, sixty["n_lines"], sixty["w"])
    other = int(nxt[(at + 1) % 6])
    with pytest.raises(ValueError) as e:
        neg.explain_by_sample([other], [[other, int(nxt[at])]], 5)
    assert "sample id %d " % nxt[at] in str(e.value) and "line %d" % bad[at][0][len(bad[at][1]) // 2] in str(e.value)
    with pytest.raises(ValueError) as e:
        neg.explain_by_sample([int(nxt[at])], [[other]], 5)
    assert "sample id %d " % nxt[at] in str(e.value) and "negative coverage" in str(e.value)
    # weights not set
    l, c = rows[0]
    bare = JunctionStore.from_arrays(np.array([1], np.int64), np.array([0, len(l)], np.int64), l, c, sixty["n_lines"])
    with pytest.raises(RuntimeError) as e:
        bare.explain_by_sample([1], [[1]], 5)
    assert "weights" in str(e.value)
