"""`morna labels` on the command line, on the 600-sample cohort of test_gpu_restrict_cli.py: every printed
number is recomputed here from the arrays of MornaSearch.label_separation with the formulas of the contract (whole text), and
those arrays are checked against fp64 numpy over the index's rows (morna_get_items) within the bound derived from the scan's
own error bound.  -m gpu"""
import numpy as np
import pytest

from test_gpu_junctions import run_cli
from test_gpu_restrict_cli import N_INDEX, cohort  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

ONE = 2.0 ** 32


@pytest.fixture(scope="module")
def tissues(cohort):  # noqa: F811
    """liver 200 samples, brain 180, heart one sample (a query: nothing of its own label is left to it), `none` empty; the
    other 219 samples carry no label."""
    ids = cohort["ids"]
    lonely = cohort["queries"][2]
    rest = [s for s in ids if s != lonely]
    labels = [("liver", rest[:200]), ("brain", rest[200:380]), ("heart", [lonely]), ("none", [])]
    path = str(cohort["dir"] / "tissues.tsv")
    with open(path, "w") as fh:
        fh.write("".join("%s\t%s\n" % (name, ",".join(map(str, members))) for name, members in labels))
    from morna_amd.search import MornaSearch
    searcher = MornaSearch(cohort["base"])
    item_label = np.full(N_INDEX, -1, np.int32)
    for g, (_, members) in enumerate(labels):
        item_label[[cohort["id_map"][s] for s in members]] = g
    X = searcher.annoy_index.get_items().astype(np.float64)
    return dict(path=path, labels=labels, names=[name for name, _ in labels], searcher=searcher, item_label=item_label, X=X)


def cell(v):
    if v is None:
        return "nan"
    return "%.6f" % v if isinstance(v, float) else str(v)


def line(*cells):
    return "\t".join(cell(c) for c in cells) + "\n"


def expected_text(ids, names, own, sums, counts, top=3, matrix=False, summary_only=False):
    """The whole output from the arrays: m = sums / 2^32 / counts; the nearest labels by (m, file order); for a query whose
    own label o is counted beside another, a = m[o], b = the smallest other m, s = (b - a) / max(a, b) (0 when both are 0),
    agree = the nearest label is o; the table over all queries; the label map."""
    L = len(names)
    out, silhouettes, predicted, M = [], [], [], [[[] for _ in range(L)] for _ in range(L)]
    for q, query_id in enumerate(ids):
        m = [int(sums[q][g]) / ONE / int(counts[q][g]) if counts[q][g] > 0 else None for g in range(L)]
        order = sorted((g for g in range(L) if m[g] is not None), key=lambda g: (m[g], g))
        predicted.append(order[0] if order else None)
        o = None if own is None or own[q] < 0 else int(own[q])
        if not summary_only:
            out.append("# query %s\tlabel %s\n" % (query_id, names[o] if o is not None else "-"))
            for rank, g in enumerate(order[:top]):
                out.append(line("%d." % (rank + 1), names[g], int(counts[q][g]), m[g]))
        if o is not None:
            for g in range(L):
                if m[g] is not None:
                    M[o][g].append(m[g])
        others = [g for g in order if g != o]
        if o is None or m[o] is None or not others:
            silhouettes.append(None)
            continue
        a, b = m[o], m[others[0]]
        s = (b - a) / max(a, b) if max(a, b) > 0 else 0.0
        silhouettes.append((o, a, b, s, order[0] == o))
        if not summary_only:
            out.append(line("silhouette", names[o], int(counts[q][o]), a, names[others[0]], b, s, 1 if order[0] == o else 0))
    out.append("# all %d queries\n" % len(ids))
    if own is None:
        for g in range(L):
            out.append(line(names[g], sum(1 for p in predicted if p == g)))
    else:
        defined = [x for x in silhouettes if x is not None]
        for name, group in [(names[g], [x for x in defined if x[0] == g]) for g in range(L)] + [("all", defined)]:
            if group:
                n = len(group)
                agree = sum(1 for x in group if x[4])
                out.append(line(name, n, sum(x[1] for x in group) / n, sum(x[2] for x in group) / n, sum(x[3] for x in group) / n,
                                agree, float(agree) / n))
        if len(defined) < len(ids):
            out.append("# %d queries without a silhouette\n" % (len(ids) - len(defined)))
    if matrix:
        out.append("# label map\n")
        for a in range(L):
            out.append(line(names[a], *[sum(M[a][b]) / len(M[a][b]) if M[a][b] else None for b in range(L)]))
    return "".join(out)


def check_against_numpy(t, table, Q, self_items=None, eligible=None):
    """counts exactly, sums within the derived bound of the fp64 distances over the rows morna_get_items returns."""
    X, labels = t["X"], t["item_label"]
    e = table.stats["scan_eps"]
    assert 0 < e < 1e-4
    norm = np.sqrt((X * X).sum(axis=1))
    qn = np.sqrt((Q * Q).sum(axis=1))
    ppqq = qn[:, None] * norm[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(ppqq > 0, 2.0 - 2.0 * (Q @ X.T) / ppqq, 2.0)
    for q in range(len(Q)):
        counted = labels >= 0
        if eligible is not None:
            counted = counted & eligible[q]
        if self_items is not None:
            counted = counted.copy()
            counted[self_items[q]] = False
        for g in range(len(t["names"])):
            rows = counted & (labels == g)
            assert table.counts[q, g] == rows.sum(), (q, g)
            ref = np.sqrt(np.maximum(v[q, rows], 0.0)).sum()
            bound = (np.sqrt(np.maximum(v[q, rows] + e, 0.0)) - np.sqrt(np.maximum(v[q, rows] - e, 0.0))).sum() \
                + rows.sum() * 2.0 ** -32 + 1e-9
            assert abs(int(table.sums[q, g]) / ONE - ref) <= bound, (q, g)


def test_all_items_with_the_label_map(cohort, tissues):  # noqa: F811
    t = tissues
    base = ["labels", "-x", cohort["base"], "--labels", t["path"]]
    rc, out, _ = run_cli(base + ["--all", "--matrix"])
    assert rc == 0
    inv = cohort["inv"]
    ids = [inv[i] for i in range(N_INDEX)]
    table = t["searcher"].label_separation(list(range(N_INDEX)), t["labels"])
    assert (table.item_label == t["item_label"]).all() and (table.own == t["item_label"]).all()
    assert out == expected_text(ids, t["names"], table.own, table.sums, table.counts, matrix=True)
    check_against_numpy(t, table, t["X"], self_items=np.arange(N_INDEX))
    # the lonely sample is the only `heart`: no silhouette for it, and heart's row of the map holds what it alone measured
    q = cohort["id_map"][cohort["queries"][2]]
    assert table.counts[q].tolist() == [200, 180, 0, 0]
    assert "# query %d\tlabel heart\n1." % cohort["queries"][2] in out and "# 220 queries without a silhouette\n" in out
    assert out.rstrip("\n").split("\n")[-1].startswith("none\tnan\tnan\tnan\tnan")
    # --summary-only prints the tail of the same text
    rc, short, _ = run_cli(base + ["--all", "--matrix", "--summary-only"])
    assert rc == 0 and short == out[out.index("# all %d queries\n" % N_INDEX):]
    assert short == expected_text(ids, t["names"], table.own, table.sums, table.counts, matrix=True, summary_only=True)


def test_sample_is_reproducible_and_query_ids_with_top(cohort, tissues):  # noqa: F811
    t = tissues
    base = ["labels", "-x", cohort["base"], "--labels", t["path"]]
    rc, out, _ = run_cli(base + ["--sample", "25", "--sample-seed", "3"])
    rc2, again, _ = run_cli(base + ["--sample", "25", "--sample-seed", "3"])
    rc3, other, _ = run_cli(base + ["--sample", "25", "--sample-seed", "4"])
    assert rc == 0 and rc2 == 0 and rc3 == 0 and out == again and out != other
    picked = np.random.RandomState(3).choice(N_INDEX, size=25, replace=False)
    table = t["searcher"].label_separation([int(i) for i in picked], t["labels"])
    assert out == expected_text([cohort["inv"][int(i)] for i in picked], t["names"], table.own, table.sums, table.counts)
    check_against_numpy(t, table, t["X"][picked], self_items=picked)
    # --query-ids, -q and --top
    queries = cohort["queries"]
    internal = [cohort["id_map"][s] for s in queries]
    table = t["searcher"].label_separation(internal, t["labels"])
    for top in (1, 2, 4):
        rc, out, _ = run_cli(base + ["--query-ids", ",".join(map(str, queries)), "--top", str(top)])
        assert rc == 0 and out == expected_text(queries, t["names"], table.own, table.sums, table.counts, top=top)
    rc, out, _ = run_cli(base + ["-q", str(queries[0])])
    assert rc == 0 and out == expected_text(queries[:1], t["names"], table.own[:1], table.sums[:1], table.counts[:1])
    with pytest.raises(ValueError, match="424242"):
        run_cli(base + ["--query-ids", "424242"])


def test_leave_out_groups_and_within(cohort, tissues):  # noqa: F811
    t = tissues
    queries = cohort["queries"]
    internal = np.array([cohort["id_map"][s] for s in queries])
    base = ["labels", "-x", cohort["base"], "--labels", t["path"], "--query-ids", ",".join(map(str, queries))]
    rc, plain, _ = run_cli(base)
    assert rc == 0
    # --leave-out-groups: the first query's donor group of 40 and the second's of 2 are not counted; the third, which the file
    # does not name, is a group of its own
    rc, out, err = run_cli(base + ["--leave-out-groups", cohort["groups_file"]])
    assert rc == 0 and out != plain
    assert "restriction: %d of %d samples allowed, 4 leave-out groups\n" % (N_INDEX, N_INDEX) in err
    groups = list(cohort["groups"]) + [("query-%d" % queries[2], [queries[2]])]
    restriction = t["searcher"].restriction(groups=groups)
    table = t["searcher"].label_separation(internal.tolist(), t["labels"], restriction=restriction)
    assert out == expected_text(queries, t["names"], table.own, table.sums, table.counts)
    item_group = restriction.item_group
    eligible = np.stack([item_group != item_group[i] for i in internal])
    check_against_numpy(t, table, t["X"][internal], self_items=internal, eligible=eligible)
    donor = set(cohort["id_map"][s] for s in cohort["groups"][0][1])
    labelled_donor = sum(1 for i in donor if t["item_label"][i] >= 0 and i != internal[0])
    unrestricted = t["searcher"].label_separation(internal.tolist(), t["labels"])
    assert labelled_donor > 0 and unrestricted.counts[0].sum() - table.counts[0].sum() == labelled_donor
    # --within: a third of the index
    rc, out, err = run_cli(base + ["--within", cohort["some_file"]])
    assert rc == 0 and "restriction: %d of %d samples allowed, 0 leave-out groups\n" % (len(cohort["some"]), N_INDEX) in err
    restriction = t["searcher"].restriction(within=cohort["some"])
    table = t["searcher"].label_separation(internal.tolist(), t["labels"], restriction=restriction)
    assert out == expected_text(queries, t["names"], table.own, table.sums, table.counts)
    check_against_numpy(t, table, t["X"][internal], self_items=internal, eligible=np.tile(restriction.allow, (3, 1)))
    # --without the same list: the two halves add up to the whole, integer for integer
    rc, rest, _ = run_cli(base + ["--without", cohort["some_file"]])
    other = t["searcher"].label_separation(internal.tolist(), t["labels"], restriction=t["searcher"].restriction(without=cohort["some"]))
    assert rc == 0 and rest == expected_text(queries, t["names"], other.own, other.sums, other.counts)
    assert (table.sums + other.sums == unrestricted.sums).all() and (table.counts + other.counts == unrestricted.counts).all()


def test_queries_from_outside_the_index(cohort, tissues):  # noqa: F811
    t = tissues
    base = ["labels", "-x", cohort["base"], "--labels", t["path"]]
    rc, out, _ = run_cli(base + ["--intropolis", cohort["queries_file"]])
    assert rc == 0
    batch = t["searcher"].queries_from_intropolis(cohort["queries_file"])
    table = t["searcher"].label_separation(batch, t["labels"])
    assert table.own is None and len(batch.ext_ids) >= 3
    assert out == expected_text(batch.ext_ids, t["names"], None, table.sums, table.counts)
    assert "silhouette" not in out and "\tlabel -\n" in out
    r64, _ = t["searcher"].annoy_index.get_query_rows()
    check_against_numpy(t, table, r64)
    rc, short, _ = run_cli(base + ["--intropolis", cohort["queries_file"], "--summary-only"])
    assert rc == 0 and short == out[out.index("# all "):]
    # a query on stdin, -f raw: every seventh junction of the indexed file, covered five times
    raw = "".join("%s\t5\n" % "\t".join(text.split("\t")[:3]) for text in cohort["lines"][::7])
    rc, out, _ = run_cli(base + ["-f", "raw"], stdin_text=raw)
    assert rc == 0
    from morna_amd.search import MornaSearch
    fresh = MornaSearch(cohort["base"])
    for text in cohort["lines"][::7]:
        tokens = text.split("\t")
        if " ".join(tokens[:3]) in fresh.sample_frequencies:
            fresh.update_query((tokens[0], int(tokens[1]), int(tokens[2]), 5))
    fresh.finalize_query()
    Q = np.array([fresh.query_sample], np.float64)
    assert Q.any()
    table = t["searcher"].label_separation(Q, t["labels"])
    assert out == expected_text(["stdin"], t["names"], None, table.sums, table.counts)
    check_against_numpy(t, table, Q)


def test_search_output_is_unchanged(cohort, tissues):  # noqa: F811
    """The same `search` commands before and after a `labels` run on the same index give the same bytes."""
    q = cohort["queries"][0]
    commands = [["search", "-x", cohort["base"], "-d", "-q", str(q)], ["search", "-x", cohort["base"], "-d", "-e", "--query-ids",
                ",".join(map(str, cohort["queries"]))], ["search", "-x", cohort["base"], "-d", "-e", "--intropolis", cohort["queries_file"]]]
    before = [run_cli(c) for c in commands]
    assert run_cli(["labels", "-x", cohort["base"], "--labels", tissues["path"], "--all", "--summary-only"])[0] == 0
    assert [run_cli(c) for c in commands] == before
    # and within one process: an exact search on the searcher that made the tables
    s = tissues["searcher"]
    items = np.arange(40, dtype=np.int32)
    first = s.annoy_index.exact_search_by_item_batch(items, 10)
    s.label_separation(list(range(N_INDEX)), tissues["labels"])
    for x, y in zip(first, s.annoy_index.exact_search_by_item_batch(items, 10)):
        assert x.tobytes() == y.tobytes()
