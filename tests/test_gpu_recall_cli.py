"""`morna recall` and `search --use-trees` on the command line, on the synthetic cohort of the restricted
CLI tests.  Every cell line of `recall` is derived again from the printed lists of separate `search --use-trees t --search-k
s` and `search -e` runs (for queries that are samples of the index, whose exact search the `search` command does not offer
by id, from exact_search_by_item_batch); the summary block from the per-query lines.  Whole text.  -m gpu"""
import numpy as np
import pytest

from test_gpu_junctions import blocks, result_ids, run_cli
from test_gpu_restrict_cli import N_INDEX, TREES, cohort  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

R = 20
TREE_LIST = (1, 3, TREES)
SEARCH_KS = (10, 100, 2000)


def cell_lines(text):
    """{query: [fields of every cell line]} of the per-query blocks, and the lines of the summary block."""
    head, _, tail = text.partition("# all ")
    per_query = {q: [line.split("\t") for line in body.splitlines()] for q, body in blocks(head)}
    return per_query, tail.splitlines()


def expected_block(approx, exact_ids, candidates, dots):
    """The cell lines of one query from its result lists: approx[(t, s)] and exact_ids are lists of internal ids; exact_ids
    None: the exact search failed for the query (count -1)."""
    lines = []
    for i, t in enumerate(TREE_LIST):
        for j, s in enumerate(SEARCH_KS):
            if exact_ids is None:
                lines.append([str(t), str(s), "-1", "-1", "nan", str(candidates[i][j]), str(dots[i][j])])
                continue
            hits = len(set(approx[(t, s)]) & set(exact_ids))
            lines.append([str(t), str(s), str(hits), str(len(exact_ids)), "%.6f" % (float(hits) / len(exact_ids)),
                          str(candidates[i][j]), str(dots[i][j])])
    return lines


def check_summary(per_query, order, summary):
    assert summary[0] == "%d queries" % len(order)
    n_cells = len(TREE_LIST) * len(SEARCH_KS)
    rows = summary[1:1 + n_cells]
    counted = [q for q in order if per_query[q][0][2] != "-1"]
    assert counted, "the exact search failed for every query"
    assert summary[1 + n_cells:] == (["# exact search failed for %d queries" % (len(order) - len(counted))]
                                     if len(counted) < len(order) else [])
    for c, row in enumerate(rows):
        cells = [per_query[q][c] for q in counted]
        recalls = [float(int(x[2])) / int(x[3]) for x in cells]
        want = [cells[0][0], cells[0][1], "%.6f" % (sum(recalls) / len(recalls)), "%.6f" % min(recalls),
                str(sum(1 for r in recalls if r == 1.0)), "%.6f" % (float(sum(int(x[5]) for x in cells)) / len(cells)),
                "%.6f" % (float(sum(int(x[6]) for x in cells)) / len(cells))]
        assert row.split("\t") == want, c


def test_recall_of_intropolis_queries(cohort):
    common = ["-x", cohort["base"], "--intropolis", cohort["queries_file"]]
    grid = ["--trees", ",".join(map(str, TREE_LIST[:-1])) + ",all", "--search-ks", ",".join(map(str, SEARCH_KS))]
    rc, got, _ = run_cli(["recall"] + common + ["-r", str(R)] + grid)
    assert rc == 0
    per_query, summary = cell_lines(got)
    rc, exact, _ = run_cli(["search", "-e"] + common + ["-r", str(R)])
    assert rc == 0
    exact_ids = {q: result_ids(body) for q, body in blocks(exact)}
    approx = {}
    for t in TREE_LIST:
        for s in SEARCH_KS:
            rc, out, _ = run_cli(["search"] + common + ["-r", str(R), "--use-trees", str(t), "--search-k", str(s)])
            assert rc == 0
            for q, body in blocks(out):
                approx.setdefault(q, {})[(t, s)] = result_ids(body)
    order = [q for q, _ in blocks(exact)]
    assert [q for q, _ in blocks(got.partition("# all ")[0])] == order and len(order) >= 3
    from morna_amd.search import MornaSearch
    searcher = MornaSearch(cohort["base"])
    searcher.queries_from_intropolis(cohort["queries_file"])
    sweep = searcher.annoy_index.search_sweep(R, TREE_LIST, SEARCH_KS, lists=False)
    for n, q in enumerate(order):
        assert per_query[q] == expected_block(approx[q], exact_ids[q], sweep["ncand"][:, :, n], sweep["ndots"][:, :, n]), q
    check_summary(per_query, order, summary)
    rc, only, _ = run_cli(["recall"] + common + ["-r", str(R), "--summary-only"] + grid)
    assert rc == 0 and only == "# all " + got.partition("# all ")[2]


def test_recall_of_indexed_samples(cohort):
    queries = cohort["queries"]
    ids = ",".join(map(str, queries))
    grid = ["--trees", ",".join(map(str, TREE_LIST)), "--search-ks", ",".join(map(str, SEARCH_KS))]
    rc, got, _ = run_cli(["recall", "-x", cohort["base"], "--query-ids", ids, "-r", str(R)] + grid)
    assert rc == 0
    per_query, summary = cell_lines(got)
    from morna_amd.search import MornaSearch
    searcher = MornaSearch(cohort["base"])
    internal = np.array([cohort["id_map"][q] for q in queries], np.int32)
    ex_ids, _, ex_cnt = searcher.annoy_index.exact_search_by_item_batch(internal, R)
    assert ((ex_cnt == R) | (ex_cnt == -1)).all()
    sweep = searcher.annoy_index.search_sweep(R, TREE_LIST, SEARCH_KS, items=internal, lists=False)
    approx = {q: {} for q in queries}
    for t in TREE_LIST:
        for s in SEARCH_KS:
            rc, out, _ = run_cli(["search", "-x", cohort["base"], "--query-ids", ids, "-r", str(R), "--use-trees", str(t),
                                  "--search-k", str(s)])
            assert rc == 0
            for q, body in blocks(out):
                approx[q][(t, s)] = result_ids(body)
    for n, q in enumerate(queries):
        assert per_query[q] == expected_block(approx[q], ex_ids[n].tolist() if ex_cnt[n] >= 0 else None, sweep["ncand"][:, :, n],
                                              sweep["ndots"][:, :, n]), q
    check_summary(per_query, queries, summary)
    # -q is --query-ids of one
    rc, one, _ = run_cli(["recall", "-x", cohort["base"], "-q", str(queries[1]), "-r", str(R)] + grid)
    assert rc == 0 and cell_lines(one)[0] == {queries[1]: per_query[queries[1]]}
    # the single-query forms of search --use-trees print what the batch form prints for that query
    for flags in (["--use-trees", "3", "--search-k", "100"], ["--use-trees", "1"]):
        rc, single, _ = run_cli(["search", "-x", cohort["base"], "-q", str(queries[0]), "-r", str(R), "-d"] + flags)
        rc2, batch, _ = run_cli(["search", "-x", cohort["base"], "--query-ids", str(queries[0]), "-r", str(R), "-d"] + flags)
        assert rc == 0 and rc2 == 0 and blocks(batch)[0][1] == single


def test_sample_is_reproducible(cohort):
    grid = ["--trees", "1,all", "--search-ks", "50,500", "-r", "10"]
    rc, one, _ = run_cli(["recall", "-x", cohort["base"], "--sample", "7", "--sample-seed", "3"] + grid)
    rc2, two, _ = run_cli(["recall", "-x", cohort["base"], "--sample", "7", "--sample-seed", "3"] + grid)
    rc3, other, _ = run_cli(["recall", "-x", cohort["base"], "--sample", "7", "--sample-seed", "4"] + grid)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and one == two and one != other
    picked = np.random.RandomState(3).choice(N_INDEX, size=7, replace=False)
    assert [q for q, _ in blocks(one.partition("# all ")[0])] == [cohort["inv"][int(i)] for i in picked]
    rc, named, _ = run_cli(["recall", "-x", cohort["base"], "--query-ids", ",".join(str(cohort["inv"][int(i)]) for i in picked)] + grid)
    assert rc == 0 and named == one
    with pytest.raises(ValueError):
        run_cli(["recall", "-x", cohort["base"], "--sample", str(N_INDEX + 1)] + grid)
    with pytest.raises(ValueError):
        run_cli(["recall", "-x", cohort["base"], "--sample", "3", "--trees", "1,%d" % (TREES + 1), "--search-ks", "50"])
    with pytest.raises(ValueError):
        run_cli(["recall", "-x", cohort["base"], "-q", "-12345"] + grid)


def test_search_without_the_flag_is_unchanged(cohort):
    """`search` without --use-trees prints what it printed before: the lists of the library's plain calls, and what
    --use-trees <all trees> prints."""
    from morna_amd.search import MornaSearch, results_output
    import io
    ids = ",".join(map(str, cohort["queries"]))
    for query in (["--query-ids", ids], ["--intropolis", cohort["queries_file"]], ["-q", str(cohort["queries"][2])]):
        for extra in ([], ["--search-k", "300"]):
            rc, plain, _ = run_cli(["search", "-x", cohort["base"], "-d", "-r", "7"] + query + extra)
            rc2, whole, _ = run_cli(["search", "-x", cohort["base"], "-d", "-r", "7", "--use-trees", str(TREES)] + query + extra)
            assert rc == 0 and rc2 == 0 and plain == whole and len(result_ids(plain)) >= 7
    searcher = MornaSearch(cohort["base"])
    internal = np.array([cohort["id_map"][q] for q in cohort["queries"]], np.int32)
    lst, d, cnt = searcher.annoy_index.get_nns_by_item_batch(internal, 7, 100)
    rc, plain, _ = run_cli(["search", "-x", cohort["base"], "-d", "-r", "7", "--query-ids", ids])
    for n, (q, body) in enumerate(blocks(plain)):
        want = io.StringIO()
        results_output(([int(x) for x in lst[n, :cnt[n]]], [float(x) for x in d[n, :cnt[n]]]), want)
        assert body.endswith(want.getvalue())
