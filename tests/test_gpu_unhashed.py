"""`morna search --unhashed` on the GPU: ids and distances bit-identical to the restatement of the
contract in test_unhashed_cpu.py (RefUnhashed: numpy, one rounding per operation, fed the text lines), through the
command line, MornaSearch and JunctionStore.  -m gpu"""
import os

import numpy as np
import pytest

from test_gpu_junctions import _write_gz, blocks, run_cli
from test_unhashed_cpu import RefUnhashed, ref_items, ref_query_terms, ref_rows, ref_weights

pytestmark = pytest.mark.gpu

N, J, THRESHOLD, CLUSTERS = 300, 2000, 8, 6
QT = 16                      # queries per pass at 2000 lines (choose_qt, csrc/nearest.hip): asserted from nearest_stats


def ext_id(s):
    return 1000 + 7 * s


def cohort_lines(seed=20240611):
    """300 samples x 2000 lines: six clusters of line-presence probabilities (a tenth of the lines rare, under the
    threshold of 8), lognormal coverages; about 500 entries per row.  Samples 90001 and 90002 sit on lines under the
    threshold only: in the store, not in the index.  A line lists its samples in a shuffled order."""
    rng = np.random.default_rng(seed)
    prob = rng.uniform(0.0, 0.5, size=(CLUSTERS, J))
    rare = rng.random(J) < 0.1
    prob[:, rare] *= 0.03
    present = rng.random((N, J)) < prob[np.arange(N) % CLUSTERS]
    cov = np.minimum(np.ceil(rng.lognormal(1.0, 1.5, size=(N, J))), 1e6).astype(np.int64)
    lines, outsiders = [], 0
    for j in range(J):
        who = np.nonzero(present[:, j])[0]
        if len(who) == 0:
            who = np.array([j % N])
        who = rng.permutation(who)
        samples = [ext_id(int(s)) for s in who]
        covs = [int(cov[s, j]) for s in who]
        if len(who) + 2 < THRESHOLD and outsiders < 5:
            samples += [90001, 90002]
            covs += [3, 1 + outsiders]
            outsiders += 1
        lines.append("chr%d\t%d\t%d\t+\tGT\tAG\t%s\t%s\n" % (1 + j % 22, 1000 + 10 * j, 1500 + 10 * j, ",".join(map(str, samples)),
                                                           ",".join(map(str, covs))))
    assert outsiders == 5
    return lines


def reference(lines, sample_count, threshold):
    """(items in internal-id order, rows by sample id, weights, RefUnhashed over the items)."""
    items, rows, w = ref_items(lines, threshold), ref_rows(lines), ref_weights(lines, sample_count, threshold)
    return items, rows, w, RefUnhashed([rows[s] for s in items], w)


def expected_text(order, dist, meta=None):
    """What results_output writes for one result: rank, id, distance (and the metadata tuple)."""
    out = []
    for r, (i, d) in enumerate(zip(order, dist)):
        out.append("%d.\t%s\t%s%s\n" % (r + 1, i, d, "" if meta is None else "\t" + str(meta[r])))
    return "".join(out)


def assert_same(got, ref, q_lines, q_cov, k, distances=None):
    """One query's (ids, distances, count) against the restatement, bit for bit, with the padding.  distances: the
    restatement's distance to every row of the population, where a fixture has made them already."""
    ids, d, cnt = got
    if distances is None:
        order, dist = ref.nearest(q_lines, q_cov, k)
    else:
        order = sorted(range(len(distances)), key=lambda i: (distances[i], -i))[:k]
        dist = [float(distances[i]) for i in order]
    m = len(order)
    assert int(cnt) == m == min(k, ref.n)
    assert ids[:m].tolist() == order
    assert d[:m].tobytes() == np.array(dist, np.float64).tobytes()
    assert (ids[m:] == -1).all() and np.isposinf(d[m:]).all()


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    d = tmp_path_factory.mktemp("unhashed")
    lines = cohort_lines()
    src, base, meta = str(d / "junctions.gz"), str(d / "idx"), str(d / "meta.tsv")
    _write_gz(src, lines)
    with open(meta, "w") as fh:
        for s in range(N):
            fh.write("%d\tsample%d cluster%d\n" % (ext_id(s), s, s % CLUSTERS))
    rc, _, _ = run_cli(["index", "--intropolis", src, "-x", base, "--features", "64", "--n-trees", "4", "-s", str(N + 2),
                        "-t", str(THRESHOLD), "-m", meta, "--junction-store"])
    assert rc == 0 and os.path.exists(base + ".jw.mor")
    items, rows, w, ref = reference(lines, N + 2, THRESHOLD)
    assert len(items) == N and 90001 in rows and 90001 not in items
    rad = np.array([ref.radicands(*rows[s]) for s in items])                 # every item as the query: [query][row]
    from morna_amd.search import MornaSearch
    return dict(dir=d, src=src, base=base, lines=lines, items=items, rows=rows, w=w, ref=ref, rad=rad,
                dist=np.sqrt(np.maximum(rad, 0.0)), searcher=MornaSearch(base))


@pytest.fixture(scope="module")
def generic(tmp_path_factory, embedded):
    d = tmp_path_factory.mktemp("unhashed_generic")
    src, base = str(d / "junctions.gz"), str(d / "idx")
    _write_gz(src, embedded["generic"])
    rc, _, _ = run_cli(["index", "--intropolis", src, "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "2",
                        "--junction-store"])
    assert rc == 0
    items, rows, w, ref = reference(embedded["generic"], 10, 2)
    return dict(src=src, base=base, lines=embedded["generic"], items=items, rows=rows, w=w, ref=ref)


# ---- the fixtures through the command line and MornaSearch -------------------------------------------------------------
def test_generic_every_sample_as_q(generic):
    from morna_amd.junctions import load_weights
    from morna_amd.search import MornaSearch
    w, sample_count, threshold = load_weights(generic["base"] + ".jw.mor", len(generic["lines"]))
    assert w.tobytes() == generic["w"].tobytes() and (sample_count, threshold) == (10, 2)
    assert MornaSearch(generic["base"]).internal_id_map == {s: i for i, s in enumerate(generic["items"])}
    ref, items = generic["ref"], generic["items"]
    assert len(items) == 10
    for i, s in enumerate(items):
        rc, out, _ = run_cli(["search", "-x", generic["base"], "--unhashed", "-q", str(s), "-d", "-r", "3"])
        assert rc == 0
        order, dist = ref.nearest(*generic["rows"][s], k=3)
        assert out == "querying by sample id %d\nthis is internal id %d\n" % (s, i) + expected_text(order, dist)
    for k in (1, 25):                                                           # 25: more than the 10 items
        rc, out, _ = run_cli(["search", "-x", generic["base"], "--unhashed", "--query-ids", ",".join(map(str, items)), "-d",
                              "-r", str(k)])
        assert rc == 0
        got = blocks(out)
        assert [s for s, _ in got] == items
        for i, (s, text) in enumerate(got):
            order, dist = ref.nearest(*generic["rows"][s], k=k)
            assert len(order) == min(k, 10)
            assert text == "querying by sample id %d\nthis is internal id %d\n" % (s, i) + expected_text(order, dist)


@pytest.mark.parametrize("k", [1, 10, 400])
def test_cohort_batch_sizes(cohort, k):
    s, ref, items = cohort["searcher"], cohort["ref"], cohort["items"]
    store, _ = s.unhashed_store()
    for nq in (1, QT - 1, QT, QT + 1, N):
        queries = items[:nq] if nq == N else items[5:5 + nq]
        ids, d, cnt = store.nearest_by_sample(np.array(items, np.int64), queries, k)
        stats = store.nearest_stats()
        assert stats["queries_per_pass"] == QT and stats["passes"] == -(-nq // QT)
        assert stats["bytes"] == 8 * sum(len(cohort["rows"][x][0]) for x in items) * stats["passes"]
        for q, sample in enumerate(queries):
            assert_same((ids[q], d[q], cnt[q]), ref, *cohort["rows"][sample], k=k, distances=cohort["dist"][items.index(sample)])
        results = s.unhashed_search_member_n_batch(queries, k)
        assert [r[0] for r in results] == [ids[q, :cnt[q]].tolist() for q in range(nq)]
        assert [r[1] for r in results] == [d[q, :cnt[q]].tolist() for q in range(nq)]


def test_cohort_filter_condition_and_window(cohort):
    """A condition, not a measurement: where the restatement's k-th and (k+1)-th radicands differ by more than 1e-9 for
    every query, a window of about 1e-12 leaves at most 2k candidates per query."""
    k = 10
    srt = np.sort(cohort["rad"], axis=1)
    assert (srt[:, k] - srt[:, k - 1] > 1e-9).all()
    store, _ = cohort["searcher"].unhashed_store()
    store.nearest_by_sample(np.array(cohort["items"], np.int64), cohort["items"], k)
    stats = store.nearest_stats()
    longest = max(len(cohort["rows"][s][0]) for s in cohort["items"])
    assert 0 < stats["window"] < 1e-11 and stats["window"] >= 2 * longest * 2.0 ** -53
    assert k <= stats["max_candidates"] <= 2 * k and N * k <= stats["candidates"] <= 2 * N * k
    assert stats["kernel_ms"] > 0


def test_cohort_is_deterministic_and_independent_of_qt(cohort, monkeypatch):
    s = cohort["searcher"]
    store, _ = s.unhashed_store()
    pop, queries = np.array(cohort["items"], np.int64), cohort["items"][:37]
    first = store.nearest_by_sample(pop, queries, 10)
    again = store.nearest_by_sample(pop, queries, 10)
    assert store.nearest_stats()["norms_ms"] == 0.0                          # the norms of this population are cached
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for qt in (4, 8):
        monkeypatch.setenv("MORNA_UNHASHED_QT", str(qt))
        other = store.nearest_by_sample(pop, queries, 10)
        stats = store.nearest_stats()
        assert stats["queries_per_pass"] == qt and stats["passes"] == -(-len(queries) // qt)
        for a, b in zip(first, other):
            assert a.tobytes() == b.tobytes()


def test_cohort_population_and_query_outside_the_index(cohort):
    """A population that leaves out store samples; a store sample that is not an item as the query."""
    store, _ = cohort["searcher"].unhashed_store()
    items, rows = cohort["items"], cohort["rows"]
    assert store.n_samples == N + 2
    some = [items[i] for i in range(0, N, 3)] + [90002]
    ref = RefUnhashed([rows[s] for s in some], cohort["w"])
    queries = [items[0], items[1], 90001, items[299]]
    ids, d, cnt = store.nearest_by_sample(some, queries, 12)
    assert store.nearest_stats()["norms_ms"] > 0.0                           # another population: its norms are made
    for q, sample in enumerate(queries):
        assert_same((ids[q], d[q], cnt[q]), ref, *rows[sample], k=12)
    with pytest.raises(IndexError) as e:
        store.nearest_by_sample(some + [424242], queries, 3)
    assert "424242" in str(e.value)
    with pytest.raises(IndexError) as e:
        store.nearest_by_sample(some, [items[0], 515151], 3)
    assert "515151" in str(e.value)
    with pytest.raises(IndexError):
        store.nearest_by_sample(some + [some[0]], queries, 3)               # named twice
    with pytest.raises(ValueError) as e:
        cohort["searcher"].unhashed_search_member_n_batch([items[0], 515151], 3)
    assert "515151" in str(e.value)


# ---- row lengths, ties and the domain: stores made from arrays -----------------------------------------------------------
def array_store(rows, n_lines, w):
    from morna_amd.junctions import JunctionStore
    ext = np.array([500 + 2 * i for i in range(len(rows))], np.int64)
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l, _ in rows])
    line = np.concatenate([np.asarray(l, np.int32) for l, _ in rows])
    cov = np.concatenate([np.asarray(c, np.int32) for _, c in rows])
    store = JunctionStore.from_arrays(ext, ptr, line, cov, n_lines)
    store.set_weights(w)
    return store, ext


def random_rows(rng, lengths, n_lines):
    rows = []
    for n in lengths:
        l = np.sort(rng.choice(n_lines, size=n, replace=False)).astype(np.int32)
        rows.append((l, np.ceil(rng.lognormal(1.0, 1.5, size=n)).astype(np.int32)))
    return rows


def test_row_lengths_through_from_arrays():
    rng = np.random.default_rng(7)
    n_lines = 3001
    w = np.where(rng.random(n_lines) < 0.2, 0.0, rng.uniform(0.05, 6.0, n_lines))
    lengths = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 700, 1500, 3001] + [int(x) for x in rng.integers(1, 400, 40)]
    rows = random_rows(rng, lengths, n_lines)
    rows[1] = (rows[1][0], np.array([0], np.int32))                           # a row whose only coverage is 0
    store, ext = array_store(rows, n_lines, w)
    ref = RefUnhashed(rows, w)
    for k in (1, 7, len(rows) + 3):
        ids, d, cnt = store.nearest_by_sample(ext, ext, k)
        for q in range(len(rows)):
            assert_same((ids[q], d[q], cnt[q]), ref, *rows[q], k=k)
    outside = random_rows(rng, [0, 1, 64, 65, 900, 3001], n_lines)
    ids, d, cnt = store.nearest(ext, outside, 9)
    for q, (l, c) in enumerate(outside):
        assert_same((ids[q], d[q], cnt[q]), ref, l, c, k=9)
    # an empty query (and a row without weight): every distance is sqrt(2.0), the ids descend
    assert ids[0].tolist() == list(range(len(rows) - 1, len(rows) - 10, -1))
    assert d[0].tobytes() == np.full(9, np.sqrt(2.0)).tobytes()
    ids, d, cnt = store.nearest_by_sample(ext, [ext[0]], len(rows))
    assert ids[0].tolist() == list(range(len(rows) - 1, -1, -1)) and (d[0] == np.sqrt(2.0)).all()


def test_ties_and_scaled_copies_are_reranked():
    """Two identical rows tie (higher id first); rows that are x2 and x3 copies of a row have its cosine and other
    roundings: all of them lie inside the window of the first, so more than k candidates are re-ranked."""
    rng = np.random.default_rng(11)
    n_lines = 1500
    w = rng.uniform(0.05, 6.0, n_lines)
    rows = random_rows(rng, [300] * 12, n_lines)
    base = rows[2]
    rows[5] = (base[0].copy(), base[1].copy())
    rows[7] = (base[0].copy(), base[1] * 2)
    rows[9] = (base[0].copy(), base[1] * 3)
    store, ext = array_store(rows, n_lines, w)
    ref = RefUnhashed(rows, w)
    for k in (1, 2, 3, 4, 6):
        ids, d, cnt = store.nearest_by_sample(ext, [ext[2], ext[7]], k)
        stats = store.nearest_stats()
        if k < 4:
            assert stats["max_candidates"] > k and stats["candidates"] > 2 * k
        for q, row in enumerate((2, 7)):
            assert_same((ids[q], d[q], cnt[q]), ref, *rows[row], k=k)
    ids, d, cnt = store.nearest_by_sample(ext, [ext[2]], 4)
    assert sorted(ids[0].tolist()) == [2, 5, 7, 9]
    at = {i: r for r, i in enumerate(ids[0].tolist())}
    assert d[0][at[5]] == d[0][at[2]] and at[5] < at[2]                        # the tie: the higher id first
    assert (d[0] < 1e-7).all()


def test_negative_coverages_are_refused():
    rng = np.random.default_rng(13)
    n_lines = 400
    w = rng.uniform(0.05, 6.0, n_lines)
    rows = random_rows(rng, [50] * 6, n_lines)
    rows[4][1][17] = -3
    store, ext = array_store(rows, n_lines, w)
    with pytest.raises(ValueError) as e:
        store.nearest_by_sample(ext, [ext[0]], 3)
    assert "sample id %d " % ext[4] in str(e.value) and "line %d" % rows[4][0][17] in str(e.value)
    rest = np.delete(ext, 4)
    ids, d, cnt = store.nearest_by_sample(rest, [ext[0]], 3)                  # the row is outside this population
    assert_same((ids[0], d[0], cnt[0]), RefUnhashed([rows[i] for i in (0, 1, 2, 3, 5)], w), *rows[0], k=3)
    with pytest.raises(ValueError) as e:
        store.nearest_by_sample(rest, [ext[4]], 3)                          # ... but it may not be the query either
    assert "negative coverage" in str(e.value)
    with pytest.raises(ValueError) as e:
        store.nearest(rest, [([1, 5], [2, -1])], 3)
    assert "line 5" in str(e.value)


# ---- queries from outside the index, and the command line ----------------------------------------------------------------
def test_external_queries_intropolis_and_raw_stream(cohort, tmp_path):
    lines, rows, items, w, ref = cohort["lines"], cohort["rows"], cohort["items"], cohort["w"], cohort["ref"]
    # query samples 70000.. copy indexed samples; 70003 has one junction on two lines of the query file (summed) and one
    # the index never saw
    copied = [items[3], items[100], items[299]]
    per_sample = {70000 + i: dict(zip(*rows[s])) for i, s in enumerate(copied)}
    per_sample[70003] = {5: 4, 6: 9, 900: 2}
    qlines = []
    for j in sorted(set().union(*[set(d) for d in per_sample.values()])):
        who = [s for s in sorted(per_sample) if j in per_sample[s]]
        qlines.append("\t".join(lines[j].split("\t")[:6] + [",".join(map(str, who)), ",".join(str(per_sample[s][j]) for s in who)]) + "\n")
    qlines.append("\t".join(lines[900].split("\t")[:6] + ["70003", "5"]) + "\n")
    qlines.append("chrUn\t1\t2\t+\tGT\tAG\t70003,70001\t8,8\n")
    per_sample[70003][900] += 5
    qpath = str(tmp_path / "queries.gz")
    _write_gz(qpath, qlines)
    first_seen = []
    for text in qlines:
        for s in text.split("\t")[6].split(","):
            if int(s) not in first_seen:
                first_seen.append(int(s))
    keys = [" ".join(t.split("\t")[:3]) for t in lines]
    k = 10
    rc, out, _ = run_cli(["search", "-x", cohort["base"], "--unhashed", "--intropolis", qpath, "--junction-file", cohort["src"], "-d",
                          "-r", str(k)])
    assert rc == 0
    got = blocks(out)
    assert [s for s, _ in got] == first_seen
    for s, text in got:
        terms = ref_query_terms({keys[j]: c for j, c in per_sample[s].items()}, lines, w)
        order, dist = ref.nearest([j for j, _ in terms], [c for _, c in terms], k)
        assert text == expected_text(order, dist), s
        if s < 70003:
            assert order[0] == cohort["searcher"].internal_id_map[copied[s - 70000]] and dist[0] < 1e-7
    # the same query as a raw stream: a junction named twice is summed, an unknown one dropped
    raw = "".join("%s\t%s\t%s\t%d\n" % (tuple(keys[j].split(" ")) + (c,)) for j, c in ((5, 4), (6, 9), (900, 2), (900, 5)))
    raw += "chrUn\t1\t2\t8\n"
    rc, out, _ = run_cli(["search", "-x", cohort["base"], "--unhashed", "-f", "raw", "--junction-file", cohort["src"], "-d", "-r", str(k)],
                         stdin_text=raw)
    assert rc == 0 and out == dict(got)[70003]
    other = str(tmp_path / "other.gz")
    _write_gz(other, lines[:-1])
    with pytest.raises(ValueError) as e:
        run_cli(["search", "-x", cohort["base"], "--unhashed", "-f", "raw", "--junction-file", other], stdin_text=raw)
    assert "not the file that was indexed" in str(e.value)


def test_cli_query_ids_with_distances_and_metadata(cohort):
    items, ref, rows = cohort["items"], cohort["ref"], cohort["rows"]
    queries = [items[i] for i in (0, 17, 150, 299, 42)]
    rc, out, _ = run_cli(["search", "-x", cohort["base"], "--unhashed", "--query-ids", ",".join(map(str, queries)), "-d", "-m", "-r", "6"])
    assert rc == 0
    got = blocks(out)
    assert [s for s, _ in got] == queries
    for s, text in got:
        order, dist = ref.nearest(*rows[s], k=6)
        meta = [("sample%d cluster%d\n" % ((items[i] - 1000) // 7, ((items[i] - 1000) // 7) % CLUSTERS),) for i in order]
        assert text == ("querying by sample id %d\nthis is internal id %d\n" % (s, items.index(s)) + expected_text(order, dist, meta))
    rc, one, _ = run_cli(["search", "-x", cohort["base"], "--unhashed", "-q", str(queries[1]), "-d", "-m", "-r", "6"])
    assert rc == 0 and one == got[1][1]
    rc, plain, _ = run_cli(["search", "-x", cohort["base"], "--unhashed", "-q", str(queries[1]), "-r", "6"])
    assert rc == 0 and plain.count("\t") == 6                                   # no -d: ranks and ids only


def test_repeated_junction_index_has_no_weights_and_unhashed_says_why(tmp_path, embedded):
    lines = list(embedded["generic"])
    lines.append("\t".join(lines[0].split("\t")[:6] + ["7,8", "1,1"]) + "\n")
    src, base = str(tmp_path / "junctions.gz"), str(tmp_path / "idx")
    _write_gz(src, lines)
    rc, _, err = run_cli(["index", "--intropolis", src, "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "2",
                          "--junction-store"])
    assert rc == 0 and os.path.exists(base + ".junc.mor") and not os.path.exists(base + ".jw.mor")
    assert "repeated junctions" in err
    with pytest.raises(IOError) as e:
        run_cli(["search", "-x", base, "--unhashed", "-q", "1"])
    assert "repeat" in str(e.value)
    # an index of the same basename without a store removes the weights of an earlier one too
    good = str(tmp_path / "good.gz")
    _write_gz(good, embedded["generic"])
    common = ["index", "--intropolis", good, "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "2"]
    assert run_cli(common + ["--junction-store"])[0] == 0 and os.path.exists(base + ".jw.mor")
    assert run_cli(common + ["--shards", "2", "--junction-store"])[0] == 0 and os.path.exists(base + ".jw.mor")
    rc, out, _ = run_cli(["search", "-x", base, "--unhashed", "-q", "1", "-r", "2"])      # a sharded index, one process
    assert rc == 0 and out.startswith("querying by sample id 1\n")
    assert run_cli(common)[0] == 0 and not os.path.exists(base + ".jw.mor") and not os.path.exists(base + ".junc.mor")
