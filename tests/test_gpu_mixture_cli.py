"""`morna mixture` on the command line, on the 600-sample cohort of test_gpu_restrict_cli.py with the
`tissues` table of test_gpu_labels_cli.py made again here: the whole text is recomputed from the arrays of
MornaSearch.label_mixture with the formulas of the command, those arrays are the restatement's bytes over the index's rows, a
pooled sample of two labels shows both, and `labels` and `cluster` print what they printed before.  -m gpu"""
import numpy as np
import pytest

from mixture_ref import ref_mixture
from test_gpu_junctions import run_cli
from test_gpu_restrict_cli import N_INDEX, cohort  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tissues(cohort):  # noqa: F811
    """liver 200 samples, brain 180, heart one sample (a query: nothing of its own label is left to it), `none` empty; the
    other 219 samples carry no label."""
    ids = cohort["ids"]
    lonely = cohort["queries"][2]
    rest = [s for s in ids if s != lonely]
    labels = [("liver", rest[:200]), ("brain", rest[200:380]), ("heart", [lonely]), ("none", [])]
    path = str(cohort["dir"] / "mixture_tissues.tsv")
    with open(path, "w") as fh:
        fh.write("".join("%s\t%s\n" % (name, ",".join(map(str, members))) for name, members in labels))
    from morna_amd.search import MornaSearch
    searcher = MornaSearch(cohort["base"])
    item_label = np.full(N_INDEX, -1, np.int32)
    for g, (_, members) in enumerate(labels):
        item_label[[cohort["id_map"][s] for s in members]] = g
    return dict(path=path, labels=labels, names=[name for name, _ in labels], searcher=searcher, item_label=item_label,
                X=searcher.annoy_index.get_items())


def cell(v):
    if v is None:
        return "nan"
    return "%.6f" % v if isinstance(v, float) else str(v)


def line(*cells):
    return "\t".join(cell(c) for c in cells) + "\n"


def expected_text(ids, names, own, weights, info, top=3, min_share=0.1, matrix=False, summary_only=False):
    """The whole output from the arrays: share = weight / the sum of the weights; the labels of positive weight by (-weight,
    file order); mixed when the second of them holds min_share; the table over all queries; the matrix of mean shares."""
    L = len(names)
    out, per = [], []
    for q, query_id in enumerate(ids):
        total = 0.0
        for g in range(L):
            total += float(weights[q][g])
        share = [float(weights[q][g]) / total if total > 0 else 0.0 for g in range(L)]
        order = sorted((g for g in range(L) if weights[q][g] > 0), key=lambda g: (-float(weights[q][g]), g))
        mixed = len(order) >= 2 and share[order[1]] >= min_share
        o = None if own is None or own[q] < 0 else int(own[q])
        per.append((o, share, order[0] if order else None, mixed, info[q][3] != 1))
        if not summary_only:
            out.append("# query %s\tlabel %s\tresidual %.6f\tsweeps %d\tconverged %d\n" % (
                query_id, names[o] if o is not None else "-", max(float(info[q][0]), 0.0) ** 0.5, int(info[q][2]),
                1 if info[q][3] == 1 else 0))
            for rank, g in enumerate(order[:top]):
                out.append(line("%d." % (rank + 1), names[g], float(weights[q][g]), share[g]))
            out.append(line("mixed", 1 if mixed else 0))
    out.append("# all %d queries\n" % len(ids))
    if own is None:
        for g in range(L):
            out.append(line(names[g], sum(1 for p in per if p[2] == g)))
        out.append(line("mixed", sum(1 for p in per if p[3])))
        without = sum(1 for p in per if p[2] is None)
        if without:
            out.append("# %d queries without a positive weight\n" % without)
    else:
        labelled = [p for p in per if p[0] is not None]
        for name, group in [(names[g], [p for p in labelled if p[0] == g]) for g in range(L)] + [("all", labelled)]:
            if group:
                n = len(group)
                out.append(line(name, n, sum(p[1][p[0]] for p in group) / n, sum(1 for p in group if p[2] == p[0]),
                                sum(1 for p in group if p[3]), sum(1 for p in group if p[4])))
        if len(labelled) < len(per):
            out.append("# %d queries without a label of their own\n" % (len(per) - len(labelled)))
    if matrix:
        out.append("# share matrix\n")
        for a in range(L):
            group = [p for p in per if p[0] == a]
            out.append(line(names[a], *[sum(p[1][b] for p in group) / len(group) if group else None for b in range(L)]))
    return "".join(out)


def same_as_restatement(t, table, **queries):
    want = ref_mixture(t["X"], t["item_label"], len(t["names"]), tol=1e-9, max_sweeps=10000, **queries)
    assert table.weights.tobytes() == want[0].tobytes() and table.info.tobytes() == want[1].tobytes()
    assert (table.active == want[2]).all()


def test_all_items_with_the_share_matrix(cohort, tissues):  # noqa: F811
    t = tissues
    base = ["mixture", "-x", cohort["base"], "--labels", t["path"]]
    rc, out, _ = run_cli(base + ["--all", "--matrix"])
    assert rc == 0
    ids = [cohort["inv"][i] for i in range(N_INDEX)]
    table = t["searcher"].label_mixture(list(range(N_INDEX)), t["labels"])
    assert (table.item_label == t["item_label"]).all() and (table.own == t["item_label"]).all()
    assert out == expected_text(ids, t["names"], table.own, table.weights, table.info, matrix=True)
    same_as_restatement(t, table, items=np.arange(N_INDEX))
    # the lonely sample is the only `heart`: the label is inactive for it alone, and `none` for everyone
    q = cohort["id_map"][cohort["queries"][2]]
    assert not table.active[q, 2] and table.active[np.arange(N_INDEX) != q, 2].all() and not table.active[:, 3].any()
    assert "# 219 queries without a label of their own\n" in out
    assert out.rstrip("\n").split("\n")[-1] == "none\tnan\tnan\tnan\tnan"
    assert table.stats["queries"] == N_INDEX and table.stats["open"] == int((table.info[:, 3] != 1).sum())
    assert table.stats["solve_ms"] > 0 and table.stats["sweeps"] == int(table.info[:, 2].sum())
    rc, short, _ = run_cli(base + ["--all", "--matrix", "--summary-only"])
    assert rc == 0 and short == out[out.index("# all %d queries\n" % N_INDEX):]
    assert short == expected_text(ids, t["names"], table.own, table.weights, table.info, matrix=True, summary_only=True)


def test_query_ids_top_min_share_and_the_fit_flags(cohort, tissues):  # noqa: F811
    t = tissues
    base = ["mixture", "-x", cohort["base"], "--labels", t["path"]]
    queries = cohort["queries"]
    internal = [cohort["id_map"][s] for s in queries]
    table = t["searcher"].label_mixture(internal, t["labels"])
    same_as_restatement(t, table, items=np.array(internal))
    for top, share in ((1, 0.1), (3, 0.1), (3, 0.0), (2, 0.9)):
        rc, out, _ = run_cli(base + ["--query-ids", ",".join(map(str, queries)), "--top", str(top), "--min-share", str(share)])
        assert rc == 0 and out == expected_text(queries, t["names"], table.own, table.weights, table.info, top=top, min_share=share)
    rc, out, _ = run_cli(base + ["-q", str(queries[0])])
    assert rc == 0 and out == expected_text(queries[:1], t["names"], table.own[:1], table.weights[:1], table.info[:1])
    # --tolerance and --max-sweeps reach the solver
    cut = t["searcher"].label_mixture(internal, t["labels"], tol=0.0, max_sweeps=2)
    assert (cut.info[:, 2] == 2).all() and (cut.info[:, 3] == 0).all()
    rc, out, _ = run_cli(base + ["--query-ids", ",".join(map(str, queries)), "--tolerance", "0", "--max-sweeps", "2"])
    assert rc == 0 and out == expected_text(queries, t["names"], cut.own, cut.weights, cut.info) and "converged 0" in out
    with pytest.raises(ValueError, match="424242"):
        run_cli(base + ["--query-ids", "424242"])


def test_within(cohort, tissues):  # noqa: F811
    t = tissues
    queries = cohort["queries"]
    internal = [cohort["id_map"][s] for s in queries]
    base = ["mixture", "-x", cohort["base"], "--labels", t["path"], "--query-ids", ",".join(map(str, queries))]
    rc, plain, _ = run_cli(base)
    rc2, out, err = run_cli(base + ["--within", cohort["some_file"]])
    assert rc == 0 and rc2 == 0 and out != plain
    assert "restriction: %d of %d samples allowed, 0 leave-out groups\n" % (len(cohort["some"]), N_INDEX) in err
    restriction = t["searcher"].restriction(within=cohort["some"])
    table = t["searcher"].label_mixture(internal, t["labels"], restriction=restriction)
    assert out == expected_text(queries, t["names"], table.own, table.weights, table.info)
    same_as_restatement(t, table, items=np.array(internal), allow=restriction.allow)
    # a restriction made with groups is refused by the library
    with pytest.raises(ValueError, match="holds groups"):
        t["searcher"].label_mixture(internal, t["labels"], restriction=t["searcher"].restriction(groups=cohort["groups"]))


def test_queries_from_outside_the_index(cohort, tissues):  # noqa: F811
    t = tissues
    base = ["mixture", "-x", cohort["base"], "--labels", t["path"]]
    rc, out, _ = run_cli(base + ["--intropolis", cohort["queries_file"]])
    assert rc == 0
    batch = t["searcher"].queries_from_intropolis(cohort["queries_file"])
    table = t["searcher"].label_mixture(batch, t["labels"])
    assert table.own is None and len(batch.ext_ids) >= 3
    assert out == expected_text(batch.ext_ids, t["names"], None, table.weights, table.info)
    r64, _ = t["searcher"].annoy_index.get_query_rows()
    same_as_restatement(t, table, Y=r64)
    assert "\tlabel -\t" in out and "\nmixed\t" in out
    rc, short, _ = run_cli(base + ["--intropolis", cohort["queries_file"], "--summary-only"])
    assert rc == 0 and short == out[out.index("# all "):]


def test_a_pooled_sample_of_two_labels_shows_both(cohort, tmp_path):  # noqa: F811
    """`morna supersample` pools three samples of one label and three of another; its file, fed on stdin with -f raw, is fitted
    with both labels among its --top.  The two labels are small (eight samples each) so that a label's centroid is made of its
    own samples' junctions; a third label holds two hundred other samples."""
    ids = cohort["ids"]
    a, b = ids[10:18], ids[300:308]
    rest = [s for s in ids[400:] if s not in a and s not in b][:200]
    labels = tmp_path / "three.tsv"
    labels.write_text("".join("%s\t%s\n" % (name, ",".join(map(str, members))) for name, members in (("a", a), ("b", b), ("rest", rest))))
    ids_file, pooled = tmp_path / "pool.txt", str(tmp_path / "pooled.qry")
    ids_file.write_text("".join("%d\n" % s for s in a[:3] + b[:3]))
    assert run_cli(["supersample", "-x", cohort["base"], "--sample-ids", str(ids_file), "--junction-file", cohort["index"], "-o", pooled])[0] == 0
    with open(pooled) as fh:
        raw = fh.read()
    rc, out, _ = run_cli(["mixture", "-x", cohort["base"], "--labels", str(labels), "-f", "raw", "--top", "3"], stdin_text=raw)
    assert rc == 0 and out.startswith("# query stdin\tlabel -\tresidual ")
    block = out[:out.index("# all 1 queries\n")].split("\n")
    listed = [row.split("\t")[1] for row in block[1:] if row and row[0].isdigit()]
    assert "a" in listed and "b" in listed, out
    assert "mixed\t1\n" in out


def test_labels_and_cluster_output_is_unchanged(cohort, tissues):  # noqa: F811
    """The same `labels` and `cluster` commands before and after a `mixture` run on the same index give the same bytes."""
    commands = [["labels", "-x", cohort["base"], "--labels", tissues["path"], "--all", "--matrix", "--summary-only"],
                ["labels", "-x", cohort["base"], "--labels", tissues["path"], "--query-ids", ",".join(map(str, cohort["queries"]))],
                ["cluster", "-x", cohort["base"], "-k", "5", "--seed", "3", "--summary-only"]]
    before = [run_cli(c) for c in commands]
    assert all(rc == 0 for rc, _, _ in before)
    assert run_cli(["mixture", "-x", cohort["base"], "--labels", tissues["path"], "--all", "--summary-only"])[0] == 0
    assert [run_cli(c) for c in commands] == before
    # and within one process: label sums and an assignment on the searcher that made the fits
    s = tissues["searcher"]
    items = np.arange(40, dtype=np.int32)
    first = s.annoy_index.label_sums(tissues["item_label"], 4, items=items)
    s.label_mixture(list(range(N_INDEX)), tissues["labels"])
    for x, y in zip(first, s.annoy_index.label_sums(tissues["item_label"], 4, items=items)):
        assert x.tobytes() == y.tobytes()
