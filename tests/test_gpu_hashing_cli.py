"""`morna hashing` on the GPU, on the 300-sample x 2000-line cohort of test_gpu_unhashed.py: the premise
(the rows made from the store ARE the rows `morna index --features D` makes), every cell of the table recomputed from the
lists of separately built indexes, the norm columns from the restatement, and the command's other flags.

The lists the table is recomputed from: the unhashed ones are the printed lists of `search --unhashed -q`, the forest ones the
printed lists of `search -q` on indexes built with --features 16 / 64 / 300 --n-trees 4.  The exact ones come from those same
indexes through AnnoyIndex.exact_search_by_item_batch: `search -q` answers with the forest search whether or not -e is given
(as the reference's does), so the command line prints no exact list of an indexed sample.  -m gpu"""
import os
import re

import numpy as np
import pytest

from test_gpu_junctions import _write_gz, run_cli
from test_gpu_unhashed import N, THRESHOLD, cohort_lines, reference
from test_hashrows_cpu import host_hashes, ref_hash_rows

pytestmark = pytest.mark.gpu

DIMS = [16, 64, 300]
R = 10
_RESULT = re.compile(r"^\d+\.\t(-?\d+)\t(\S+)$", re.M)


def printed_list(text):
    """(ids, distances) of the result lines of one `search -d`."""
    found = _RESULT.findall(text)
    return [int(i) for i, _ in found], [float(d) for _, d in found]


def others(ids, dists, me, r=R):
    kept = [(i, d) for i, d in zip(ids, dists) if i != me and i >= 0][:r]
    return [i for i, _ in kept], [d for _, d in kept]


def table_blocks(text):
    """{label: rows} of a `hashing` output, a row the cells of one line; the summary under the label "all"."""
    out, label = {}, None
    for line in text.splitlines():
        m = re.match(r"# query (-?\d+)$", line)
        if m or line.startswith("# all "):
            label = int(m.group(1)) if m else "all"
            assert label not in out
            out[label] = []
        else:
            out[label].append(line.split("\t"))
    return out


def close(printed, value):
    """A printed cell against its recomputed value: "-" for None, integers as they are, floats to the six digits printed
    (half a unit of the last digit, and the few ulps two ways of summing the same numbers can differ by)."""
    if value is None:
        return printed == "-"
    if isinstance(value, int):
        return printed == str(value)
    return re.match(r"-?\d+\.\d{6}$", printed) is not None and abs(float(printed) - value) <= 5e-7 + 1e-12


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("hashing")
    lines = cohort_lines()
    src = str(d / "junctions.gz")
    _write_gz(src, lines)
    bases = {}
    for D in DIMS + [3000]:
        bases[D] = str(d / ("idx%d" % D))
        rc, _, _ = run_cli(["index", "--intropolis", src, "-x", bases[D], "--features", str(D), "--n-trees", "4", "-s", str(N + 2),
                            "-t", str(THRESHOLD)] + (["--junction-store"] if D == 64 else []))
        assert rc == 0
    assert os.path.exists(bases[64] + ".jw.mor") and not os.path.exists(bases[16] + ".junc.mor")
    items, rows, w, ref = reference(lines, N + 2, THRESHOLD)
    queries = [items[0], items[7], items[101], items[200], items[299]]
    return dict(dir=d, src=src, bases=bases, lines=lines, items=items, rows=rows, w=w, ref=ref, queries=queries,
                hashes=host_hashes(lines))


def test_rows_from_the_store_are_the_rows_of_an_index_of_that_width(world):
    from morna_amd.annoy import AnnoyIndex
    from morna_amd.junctions import line_hashes
    from morna_amd.search import MornaSearch
    searcher = MornaSearch(world["bases"][64])
    store, w = searcher.unhashed_store()
    assert w.tobytes() == world["w"].tobytes()
    population = searcher._unhashed_population()
    assert population.tolist() == world["items"]
    line_hash = line_hashes(world["src"], store.n_lines, searcher.annoy_index)
    assert line_hash.dtype == np.int32 and line_hash.tobytes() == world["hashes"].tobytes()
    assert searcher.annoy_index.get_n_items() == N                          # hashing the keys touched no item
    for D in (64, 3000):
        h = AnnoyIndex(D)
        h.add_items_from_store(store, population, line_hash)
        built = MornaSearch(world["bases"][D]).annoy_index
        assert h.get_items().tobytes() == built.get_items().tobytes()
        assert h.get_norms2().tobytes() == built.get_norms2().tobytes()
    want = ref_hash_rows([world["rows"][s] for s in world["items"]], world["w"], world["hashes"], 64)
    assert searcher.annoy_index.get_items().tobytes() == want.tobytes()


def expected_lists(world, approx):
    """(truth, exact, approx) per query: the lists with the query dropped, from the separately built indexes."""
    from morna_amd.search import MornaSearch
    internal = [world["items"].index(q) for q in world["queries"]]
    truth, exact, forest = [], {}, {}
    for q, me in zip(world["queries"], internal):
        rc, out, _ = run_cli(["search", "-x", world["bases"][64], "--unhashed", "-q", str(q), "-r", str(R + 1), "-d"])
        assert rc == 0
        truth.append(others(*printed_list(out), me=me))
    for D in DIMS:
        index = MornaSearch(world["bases"][D]).annoy_index
        ids, dist, cnt = index.exact_search_by_item_batch(np.array(internal, np.int32), R + 1)
        exact[D] = [others(ids[i, :cnt[i]].tolist(), dist[i, :cnt[i]].tolist(), me) for i, me in enumerate(internal)]
        if approx:
            forest[D] = []
            for q, me in zip(world["queries"], internal):
                rc, out, _ = run_cli(["search", "-x", world["bases"][D], "-q", str(q), "-r", str(R + 1), "-d", "--search-k", "50"])
                assert rc == 0
                forest[D].append(others(*printed_list(out), me=me))
    return truth, exact, forest


def expected_cells(truth, found):
    at = dict(zip(*found))
    shared = [(u, at[i]) for i, u in zip(*truth) if i in at]
    hits = len(shared)
    return hits, (float(hits) / len(truth[0]) if truth[0] else None), (sum(abs(h - u) for u, h in shared) / hits if hits else None)


@pytest.mark.parametrize("approx", [False, True], ids=["exact", "with_trees"])
def test_every_cell_of_the_table(world, approx):
    argv = ["hashing", "-x", world["bases"][64], "--junction-file", world["src"], "--features", "16,index,300", "--query-ids",
            ",".join(map(str, world["queries"])), "-r", str(R)] + (["--n-trees", "4", "--search-k", "50"] if approx else [])
    rc, out, _ = run_cli(argv)
    assert rc == 0
    got = table_blocks(out)
    assert list(got) == world["queries"] + ["all"]
    assert out.splitlines()[-len(DIMS) - 1] == "# all %d queries" % len(world["queries"])
    truth, exact, forest = expected_lists(world, approx)
    per_query = []
    for q, label in enumerate(world["queries"]):
        assert len(truth[q][0]) == R and len(got[label]) == len(DIMS)
        rows = []
        for cells, D in zip(got[label], DIMS):
            hits, recall, dist_err = expected_cells(truth[q], exact[D][q])
            want = [D, R, hits, recall, dist_err]
            if approx:
                a_hits, a_recall, _ = expected_cells(truth[q], forest[D][q])
                want += [a_hits, a_recall]
            assert len(cells) == len(want) and all(close(c, v) for c, v in zip(cells, want)), (label, D, cells, want)
            rows.append(cells)
        per_query.append(rows)
    assert any(int(r[2]) < R for rows in per_query for r in rows) and any(int(r[2]) > 0 for rows in per_query for r in rows)
    # the block over all queries, from the per-query lines as printed
    pop_rows = [world["rows"][s] for s in world["items"]]
    pp = world["ref"].pp
    assert (pp > 0).all()
    for i, (cells, D) in enumerate(zip(got["all"], DIMS)):
        mine = [rows[i] for rows in per_query]
        t, h = sum(int(r[1]) for r in mine), sum(int(r[2]) for r in mine)
        errs = [float(r[4]) for r in mine if r[4] != "-"]
        assert cells[0] == str(D) and cells[1] == str(t) and cells[2] == str(h)
        assert abs(float(cells[3]) - float(h) / t) <= 5e-7 + 1e-12
        assert abs(float(cells[4]) - sum(errs) / len(errs)) <= 1e-6 + 1e-12        # (each printed err is itself rounded at 5e-7)
        at = 5
        if approx:
            a = sum(int(r[5]) for r in mine)
            assert cells[5] == str(a) and abs(float(cells[6]) - float(a) / t) <= 5e-7 + 1e-12
            at = 7
        assert len(cells) == at + 2
        # the norm columns from the restatement: fp64 sums of the fp32 rows' squares, against the canonical fp32 norm the
        # command reads, which sums at most min(D, 700) non-zero squares: a relative error of at most 700 * 2^-24 = 4.2e-5
        # in the norm squared, half of it in its root; the ratios lie below 4, and their spread below 2
        x = ref_hash_rows(pop_rows, world["w"], world["hashes"], D).astype(np.float64)
        ratio = np.sqrt((x * x).sum(axis=1)) / np.sqrt(pp)
        assert ratio.max() < 4 and np.abs(ratio - ratio.mean()).max() < 2
        d_ratio = 4 * 2.1e-5
        assert abs(float(cells[at]) - ratio.mean()) <= d_ratio + 5e-7
        assert abs(float(cells[at + 1]) - ratio.var()) <= 2 * 2 * d_ratio + d_ratio ** 2 + 5e-7
    narrow, wide = float(got["all"][0][-1]), float(got["all"][-1][-1])
    assert narrow > wide > 0                                       # a wider row keeps the norms better


def test_sample_summary_only_and_the_wrong_file(world, tmp_path):
    base = ["hashing", "-x", world["bases"][64], "--junction-file", world["src"], "--features", "16,index", "-r", "5"]
    rc, full, _ = run_cli(base + ["--sample", "7", "--sample-seed", "3"])
    assert rc == 0
    picked = np.random.RandomState(3).choice(N, size=7, replace=False)
    labels = [world["items"][int(i)] for i in picked]
    assert list(table_blocks(full)) == labels + ["all"]
    rc, again, _ = run_cli(base + ["--sample", "7", "--sample-seed", "3"])
    assert rc == 0 and again == full
    rc, other, _ = run_cli(base + ["--sample", "7"])
    assert rc == 0 and list(table_blocks(other))[:-1] == [world["items"][int(i)] for i in np.random.RandomState(0).choice(N, 7, False)]
    rc, short, _ = run_cli(base + ["--sample", "7", "--sample-seed", "3", "--summary-only"])
    assert rc == 0 and short == "# all 7 queries\n" + "".join(full.splitlines(True)[-2:]) and full.endswith(short)
    rc, one, _ = run_cli(base + ["-q", str(labels[0])])
    assert rc == 0 and table_blocks(one)[labels[0]] == table_blocks(full)[labels[0]]
    with pytest.raises(ValueError, match="424243"):
        run_cli(base + ["-q", "424243"])
    with pytest.raises(ValueError, match="--sample 301: the index holds 300 samples"):
        run_cli(base + ["--sample", "301"])
    wrong = str(tmp_path / "fewer.gz")
    _write_gz(wrong, world["lines"][:-3])
    with pytest.raises(ValueError) as e:
        run_cli(base[:3] + ["--junction-file", wrong] + base[5:] + ["-q", str(labels[0])])
    assert "has 1997 lines, the junction store has 2000: it is not the file that was indexed" in str(e.value)
    with pytest.raises(IOError, match="no junction store"):
        run_cli(["hashing", "-x", world["bases"][16], "--junction-file", world["src"], "--features", "16", "-q", str(labels[0])])


def test_search_and_recall_print_what_they_printed(world):
    """The other commands around a `hashing` run on the same index: the same text before and after."""
    q = str(world["queries"][1])
    commands = [["search", "-x", world["bases"][64], "-q", q, "-d"],
                ["search", "-x", world["bases"][64], "--unhashed", "-q", q, "-d", "-r", "5"],
                ["recall", "-x", world["bases"][64], "--query-ids", ",".join(map(str, world["queries"])), "-r", "10", "--trees", "1,all",
                 "--search-ks", "10,100"]]
    before = [run_cli(c) for c in commands]
    rc, out, _ = run_cli(["hashing", "-x", world["bases"][64], "--junction-file", world["src"], "--features", "16,index", "-q", q])
    assert rc == 0 and out.startswith("# query %s\n16\t20\t" % q)
    assert [run_cli(c) for c in commands] == before
    assert all(rc == 0 for rc, _, _ in before)
    ids, _ = printed_list(before[0][1])
    assert len(ids) == 20 and before[2][1].count("# query") == 5
