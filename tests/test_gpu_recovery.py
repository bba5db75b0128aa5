"""`morna recovery` on the GPU: the library's histogram against its numpy restatement (test_recovery_cpu.ref_hist), entry
for entry; every cell of a grid against the shipped filter (`retain`); and whole tables of the command line against the
restatement fed the result lists the search itself printed.  Integers and whole text only, no tolerance.  -m gpu
Stores of more than 64 tiles, where the tile scan takes a second round: test_gpu_jstore_many_tiles.py."""
import gzip

import numpy as np
import pytest

from test_gpu_junctions import _write_gz, blocks, result_ids, run_cli
from test_junctions_cpu import sample_lists
from test_recovery_cpu import ref_hist, ref_recovery, rows_of_tables

pytestmark = pytest.mark.gpu

N_SAMPLES, EMPTY = 96, 1040                # external ids 1000 .. 1095; 1040 holds no line
GRID8 = [1, 2, 3, 5, 10, 20, 50, 1000]
GRID15 = [-7, 0, 1, 2, 3, 4, 5, 7, 10, 20, 50, 100, 1000, 10**6, 2**40]
SIZES = [1, 4095, 4096, 4097, 12290]       # one tile, both sides of the tile edge, three tiles and a remainder


def make_store(n_lines):
    """96 samples over n_lines lines at about 5 % density: coverages 1 + geometric, a share of them forced onto the grid's
    thresholds, one negative; sample 1040 empty; the first and last line and the lines at the tile edge held by someone."""
    from morna_amd.junctions import JunctionStore
    rng = np.random.Generator(np.random.PCG64(20260 + n_lines))
    ext = np.arange(1000, 1000 + N_SAMPLES, dtype=np.int64)
    rows = {}
    for i, s in enumerate(ext.tolist()):
        held = rng.random(n_lines) < 0.05
        if i % 7 == 0:
            held[[j for j in (0, 4095, 4096, n_lines - 1) if j < n_lines]] = True
        if s == EMPTY:
            held[:] = False
        line = np.nonzero(held)[0].astype(np.int64)
        cov = rng.geometric(0.2, len(line)).astype(np.int64)
        on_grid = rng.random(len(line)) < 0.2
        cov[on_grid] = rng.choice([2, 3, 5, 10, 20, 50, 1000], int(on_grid.sum()))
        rows[s] = (line, cov)
    if len(rows[1000][1]):
        rows[1000][1][0] = -7                                  # a negative coverage, on line 0
    ptr = np.zeros(N_SAMPLES + 1, np.int64)
    ptr[1:] = np.cumsum([len(rows[s][0]) for s in ext.tolist()])
    store = JunctionStore.from_arrays(ext, ptr, np.concatenate([rows[s][0] for s in ext.tolist()]),
                                      np.concatenate([rows[s][1] for s in ext.tolist()]), n_lines)
    # list 3 leaves 1005 out: the tests take that sample as its truth, and a list that held it would miss none of its lines
    lists = [[], [1000], [1007, 1040], rng.permutation(ext[ext != 1005])[:20].tolist(), rng.permutation(ext)[:63].tolist(),
             rng.permutation(ext)[:64].tolist(), [1003, 1014, 1003, 1000, 1014, 1003], [EMPTY]]
    return dict(store=store, rows=rows, n_lines=n_lines, ext=ext, lists=lists)


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    return make_store(request.param)


def want(case, lists, truths, grid):
    return np.stack([ref_hist(case["rows"], case["n_lines"], lst, t, grid) for lst, t in zip(lists, truths)])


def truth_of_sample(case, sample, min_cov):
    line, cov = case["rows"][sample]
    return line[cov >= min_cov]


def entries(case, samples):
    return sum(len(case["rows"][s][0]) for s in samples)


# ---- the histogram -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_cov", [1, 3])
def test_truth_by_sample_equals_restatement(case, min_cov):
    store, lists = case["store"], case["lists"]
    truth_ids = [1000, 1000, EMPTY, 1005, 1095, 1014, 1003, 1021]
    got = store.recovery_by_sample(lists, truth_ids, GRID15, truth_min_coverage=min_cov)
    assert got.dtype == np.int64 and got.shape == (len(lists), 2, 65, 16)
    expected = want(case, lists, [truth_of_sample(case, s, min_cov) for s in truth_ids], GRID15)
    assert np.array_equal(got, expected)
    assert got[:, 0, 0].sum() == 0
    if case["n_lines"] > 1:
        assert got[3, 1, 1:].sum() > 0 and got[3, 0].sum() > 0 and got[3, 1, 0, 0] > 0      # found, spurious and missed lines
    stats = store.recovery_stats()
    assert stats["bytes"] == 8 * (entries(case, [s for lst in lists for s in lst]) + entries(case, truth_ids))
    assert stats["workgroups"] == len(lists) * ((case["n_lines"] + 4095) // 4096) and stats["kernel_ms"] > 0


def test_truth_as_lines_equals_restatement(case):
    store, lists, n = case["store"], case["lists"], case["n_lines"]
    corners = [j for j in (0, 4095, 4096, n - 1) if j < n]
    corners = sorted(set(corners))
    truths = [[], corners, np.arange(n), case["rows"][1005][0], [], corners, np.arange(n), corners]
    filter_timers = store.timers()["retain"]
    got = store.recovery(lists, truths, GRID8)
    assert got.shape == (len(lists), 2, 65, 9)
    assert np.array_equal(got, want(case, lists, truths, GRID8))
    assert got[0].sum() == 0 and got[2, 1].sum() == n and got[7, 1, 0, 0] == len(corners)
    stats = store.recovery_stats()
    assert stats["bytes"] == 8 * entries(case, [s for lst in lists for s in lst]) + 4 * sum(len(t) for t in truths)
    assert store.timers()["retain"] == filter_timers           # the filter's two slots stay its own
    empty = store.recovery([], [], GRID8)
    assert empty.shape == (0, 2, 65, 9) and store.recovery_stats() == {"kernel_ms": 0.0, "bytes": 0, "workgroups": 0}


def test_every_cell_equals_the_shipped_filter(case):
    from morna_amd.junctions import recovery_rows
    store, lists = case["store"], case["lists"]
    frequencies, coverages = ["0", ".05", ".5", "1.0"], [1, 3, 10, 1000]
    truth_ids = [1002, 1000, 1007, 1005, 1095, 1014, 1003, EMPTY]
    truths = [set(truth_of_sample(case, s, 1).tolist()) for s in truth_ids]
    hist = store.recovery_by_sample(lists, truth_ids, coverages)
    tables = [recovery_rows(hist[q], len(lst), frequencies, coverages) for q, lst in enumerate(lists)]
    at = 0
    for f in frequencies:
        for c in coverages:
            kept = store.retain(lists, float(f), c)
            for q in range(len(lists)):
                row = tables[q][at]
                assert (row["frequency_filter"], row["coverage_filter"]) == (f, c)
                assert row["retrieved"] == len(kept[q]), (f, c, q)
                assert row["true_positive"] == len(set(kept[q].lines.tolist()) & truths[q]), (f, c, q)
                assert row["true_positive"] + row["false_negative"] == len(truths[q])
            at += 1


def test_histogram_does_not_depend_on_the_batch(case):
    store = case["store"]
    lst, other = case["lists"][3], case["lists"][5]
    one = store.recovery_by_sample([lst], [1005], GRID8)
    three = store.recovery_by_sample([other, lst, []], [1001, 1005, 1005], GRID8)
    many = store.recovery_by_sample([lst] * 64 + [other], [1005] * 64 + [1001], GRID8)
    assert np.array_equal(one[0], three[1]) and np.array_equal(three[0], many[64])
    assert all(np.array_equal(one[0], many[q]) for q in range(64))
    assert np.array_equal(one[0], store.recovery([lst], [truth_of_sample(case, 1005, 1)], GRID8)[0])


# ---- errors ----------------------------------------------------------------------------------------------------------------
def raw_recovery(store, lists, k, t_ptr, t_line, grid):
    """morna_jstore_recovery itself, past the checks of the Python method: (return code, message)."""
    from morna_amd._lib import lib, ptr
    res = np.zeros((len(lists), k), np.int64)
    n_res = np.array([len(lst) for lst in lists], np.int32)
    for q, lst in enumerate(lists):
        res[q, :len(lst)] = lst
    t_ptr, t_line, grid = np.array(t_ptr, np.int64), np.array(t_line, np.int32), np.array(grid, np.int64)
    hist = np.zeros((len(lists), 2, 65, len(grid) + 1), np.int32)
    rc = lib().morna_jstore_recovery(store._p, ptr(res), ptr(n_res), len(lists), k, ptr(t_ptr), ptr(t_line), ptr(grid), len(grid),
                                     ptr(hist))
    return rc, lib().morna_last_error().decode(), hist


def test_errors_leave_the_store_usable():
    from morna_amd._lib import E_INVALID
    case = make_store(4097)
    store, lst = case["store"], case["lists"][3]
    good = want(case, [lst], [truth_of_sample(case, 1005, 1)], GRID8)

    def still_works():
        assert np.array_equal(store.recovery_by_sample([lst], [1005], GRID8), good)
    still_works()
    for grid in ([1, 5, 5, 10], [10, 5], [3, 2**40, 7]):
        with pytest.raises(ValueError, match="ascend"):
            store.recovery_by_sample([lst], [1005], grid)
        still_works()
    for grid in (list(range(16)), []):
        with pytest.raises(ValueError, match="1 to 15"):
            store.recovery([lst], [[0]], grid)
        still_works()
    with pytest.raises(ValueError, match="64"):
        store.recovery_by_sample([[1000] * 65], [1005], GRID8)
    rc, message, _ = raw_recovery(store, [[1000] * 65], 65, [0, 0], [], GRID8)
    assert rc == E_INVALID and "64" in message
    still_works()
    with pytest.raises(ValueError, match="4097"):
        store.recovery([lst], [[0, 4097]], GRID8)              # the method's own check
    rc, message, _ = raw_recovery(store, [lst, lst], 20, [0, 1, 3], [5, 0, 4097], GRID8)
    assert rc == E_INVALID and "4097" in message and "position 1 of list 1" in message
    still_works()
    for bad in ([7, 3], [3, 3]):                               # descending, repeated
        with pytest.raises(ValueError, match="position 1 of list 1"):
            store.recovery([lst, lst], [[1, 2], bad], GRID8)
        still_works()
    rc, message, _ = raw_recovery(store, [lst, lst], 20, [0, 2, 4], [1, 2, -1, 3], GRID8)
    assert rc == E_INVALID and "position 0 of list 1" in message
    still_works()
    with pytest.raises(IndexError, match="424242"):
        store.recovery_by_sample([[1000, 424242]], [1005], GRID8)
    still_works()
    with pytest.raises(IndexError, match="515151"):
        store.recovery_by_sample([lst], [515151], GRID8)
    still_works()
    with pytest.raises(ValueError, match="one truth per result list"):
        store.recovery_by_sample([lst, lst], [1005], GRID8)
    rc, message, hist = raw_recovery(store, [lst], 20, [0, 2], [0, 4096], GRID8)     # and the raw call agrees when all is well
    assert rc == 0 and np.array_equal(hist.astype(np.int64), want(case, [lst], [[0, 4096]], GRID8))


# ---- the command line on the embedded fixture ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic(tmp_path_factory, embedded):
    d = tmp_path_factory.mktemp("recovery_generic")
    src, base = str(d / "junctions.gz"), str(d / "idx")
    _write_gz(src, embedded["generic"])
    rc, _, _ = run_cli(["index", "--intropolis", src, "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "4",
                        "--junction-store"])
    assert rc == 0
    return dict(dir=d, src=src, base=base, lines=embedded["generic"], tables=sample_lists(embedded["generic"]))


def table_text(rows_by_sample, n_lines, label, results, truth, extra, frequencies, coverages):
    """(the block `recovery` prints for one query, its rows) from the restatement."""
    from morna_amd.junctions import format_recovery_rows, recovery_rows
    rows = recovery_rows(ref_hist(rows_by_sample, n_lines, results, truth, coverages), len(results), frequencies, coverages,
                         extra_true=extra)
    return "# query %s\tresults %d\ttrue %d\n" % (label, len(results), len(truth) + extra) + format_recovery_rows(rows), rows


def summary_text(tables):
    from morna_amd.junctions import format_recovery_rows, sum_recovery_rows
    return "# all %d queries\n" % len(tables) + format_recovery_rows(sum_recovery_rows(tables))


def test_generic_leave_one_out_equals_restatement(generic):
    from morna_amd.junctions import parse_recovery_grid
    from morna_amd.search import MornaSearch
    frequencies, coverages = parse_recovery_grid()
    s = MornaSearch(generic["base"])
    inv = {v: k for k, v in s.internal_id_map.items()}
    rows_by_sample = rows_of_tables(generic["tables"])
    ids = list(range(1, 11))
    flags = ["--query-ids", ",".join(map(str, ids))]
    rc, out, _ = run_cli(["recovery", "-x", generic["base"], "-r", "5"] + flags)
    assert rc == 0
    _, searched, _ = run_cli(["search", "-x", generic["base"], "-r", "6"] + flags)
    found = blocks(searched)
    assert [q for q, _ in found] == ids
    texts, tables = [], []
    for q, body in found:
        results = [inv[i] for i in result_ids(body) if inv[i] != q][:5]
        assert len(results) == 5
        truth = generic["tables"][0][q]
        text, rows = table_text(rows_by_sample, len(generic["lines"]), q, results, truth, 0, frequencies, coverages)
        at = 0
        for f in frequencies:                                  # and the rows against the set-and-dict restatement itself
            for c in coverages:
                retrieved, tp, true = ref_recovery(generic["lines"], results, truth, float(f), c, generic["tables"])
                assert (rows[at]["retrieved"], rows[at]["true_positive"], rows[at]["false_negative"]) == (retrieved, tp, true - tp)
                at += 1
        texts.append(text)
        tables.append(rows)
    assert out == "".join(texts) + summary_text(tables)
    assert out.count("\n") == 11 * (2 + 64) and "\t0.05\t" not in out and "\n.05\t5\t1\t" in out      # frequencies as given
    rc, only, _ = run_cli(["recovery", "-x", generic["base"], "-r", "5", "--summary-only"] + flags)
    assert rc == 0 and only == summary_text(tables)
    # -q: that sample's block, from what `search -q` finds
    _, searched, _ = run_cli(["search", "-x", generic["base"], "-r", "6", "-q", "8"])
    results = [inv[i] for i in result_ids(searched) if inv[i] != 8][:5]
    text, rows = table_text(rows_by_sample, len(generic["lines"]), 8, results, generic["tables"][0][8], 0, frequencies, coverages)
    rc, out, _ = run_cli(["recovery", "-x", generic["base"], "-r", "5", "-q", "8"])
    assert rc == 0 and out == text + summary_text([rows]) and text == texts[7]
    # a truth coverage and a grid of one's own
    rc, out, _ = run_cli(["recovery", "-x", generic["base"], "-r", "5", "-q", "8", "--truth-coverage", "3", "--grid", "1.5,0:30,2,2"])
    line, cov = rows_by_sample[8]
    text, rows = table_text(rows_by_sample, len(generic["lines"]), 8, results, line[cov >= 3].tolist(), 0, ["1.5", "0"], [2, 30])
    assert 0 < (cov >= 3).sum() < len(cov)
    assert rc == 0 and out == text + summary_text([rows])
    with pytest.raises(ValueError, match="424242"):            # what `search -q` raises for an id the index lacks
        run_cli(["recovery", "-x", generic["base"], "-q", "424242"])
    with pytest.raises(ValueError, match="424242"):
        run_cli(["search", "-x", generic["base"], "-q", "424242"])


# ---- the command line on a synthetic cohort: shallow queries, deep truth -------------------------------------------------------
N_INDEX, N_QUERY, J, THRESHOLD, TREES, DIM = 600, 40, 3000, 30, 5, 128


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    from morna_amd.synth import index_and_query_files
    d = tmp_path_factory.mktemp("recovery_cohort")
    ipath, qpath = str(d / "index.tsv.gz"), str(d / "deep_all.tsv")
    index_and_query_files(ipath, qpath, N_INDEX, N_QUERY, J=J)
    base = str(d / "idx")
    assert run_cli(["index", "--intropolis", ipath, "-x", base, "--features", str(DIM), "--n-trees", str(TREES), "-t", str(THRESHOLD),
                    "--junction-store"])[0] == 0
    with gzip.open(ipath, "rt") as fh:
        lines = fh.readlines()
    with open(qpath) as fh:
        deep = fh.readlines()
    rng = np.random.Generator(np.random.PCG64(77))
    shallow = []
    for ln in deep:                                            # the same samples sequenced less deeply
        t = ln.rstrip("\n").split("\t")
        cov = rng.binomial([int(c) for c in t[7].split(",")], 0.3)
        kept = [(s, c) for s, c in zip(t[6].split(","), cov.tolist()) if c > 0]
        if kept:
            shallow.append("\t".join(t[:6] + [",".join(s for s, _ in kept), ",".join(str(c) for _, c in kept)]) + "\n")
    t = deep[0].rstrip("\n").split("\t")
    two = t[6].split(",")[:2]                                  # two junctions the indexed file lacks, in two samples each
    assert len(two) == 2
    novel = ["\t".join(["chrNovel", str(1000 * (i + 1)), str(1000 * (i + 1) + 500)] + t[3:6] + [",".join(two), "4,1"]) + "\n"
             for i in range(2)]
    deep = deep[:len(deep) // 2] + novel + deep[len(deep) // 2:]
    spath, dpath = str(d / "shallow.tsv.gz"), str(d / "deep.tsv.gz")
    _write_gz(spath, shallow)
    _write_gz(dpath, deep)
    from morna_amd.search import MornaSearch
    inv = {v: k for k, v in MornaSearch(base).internal_id_map.items()}
    key_line = {" ".join(ln.split("\t")[:3]): j for j, ln in enumerate(lines)}
    assert len(key_line) == len(lines)
    truth = {}                                                 # sample -> {key: coverage}, from the text of deep
    for ln in deep:
        t = ln.rstrip("\n").split("\t")
        for s, c in zip(t[6].split(","), t[7].split(",")):
            cell = truth.setdefault(int(s), {})
            cell[" ".join(t[:3])] = cell.get(" ".join(t[:3]), 0) + int(c)
    return dict(dir=d, index=ipath, shallow=spath, deep=dpath, base=base, lines=lines, rows=rows_of_tables(sample_lists(lines)),
                inv=inv, key_line=key_line, truth=truth, novel_samples=[int(x) for x in two])


@pytest.mark.parametrize("flags, min_cov", [([], 1), (["-e"], 3)])
def test_cohort_shallow_against_deep(cohort, flags, min_cov):
    from morna_amd.junctions import parse_recovery_grid
    frequencies, coverages = parse_recovery_grid()
    query = ["--intropolis", cohort["shallow"]] + flags
    rc, out, err = run_cli(["recovery", "-x", cohort["base"], "--truth", cohort["deep"], "--junction-file", cohort["index"],
                            "--truth-coverage", str(min_cov)] + query)
    assert rc == 0
    _, searched, _ = run_cli(["search", "-x", cohort["base"]] + query)
    found = blocks(searched)
    assert len(found) == N_QUERY
    texts, tables, extras = [], [], 0
    for sample, body in found:
        results = [cohort["inv"][i] for i in result_ids(body)]
        assert len(results) == 20
        keys = [key for key, c in cohort["truth"][sample].items() if c >= min_cov]
        truth = sorted(cohort["key_line"][key] for key in keys if key in cohort["key_line"])
        extra = sum(1 for key in keys if key not in cohort["key_line"])
        extras += extra
        text, rows = table_text(cohort["rows"], len(cohort["lines"]), sample, results, truth, extra, frequencies, coverages)
        texts.append(text)
        tables.append(rows)
    assert extras == (4 if min_cov == 1 else 2)                # "4,1": both samples at coverage 1, only the first at 3
    assert out == "".join(texts) + summary_text(tables)
    assert err.split("\n")[-2] == "%d true junctions of %s are not in %s: they count as false negatives" \
        % (extras, cohort["deep"], cohort["index"])
    total = tables and [sum(t[i]["true_positive"] for t in tables) for i in range(64)]
    assert max(total) > 0 and len(set(total)) > 1              # the grid matters, and something is recovered
    if not flags:                                              # a query sample the truth lacks is named
        with gzip.open(cohort["deep"], "rt") as fh:
            fewer = [ln for ln in fh if str(found[0][0]) not in ln.split("\t")[6].split(",")]
        other = str(cohort["dir"] / "fewer.tsv.gz")
        _write_gz(other, fewer)
        with pytest.raises(ValueError, match=str(found[0][0])):
            run_cli(["recovery", "-x", cohort["base"], "--truth", other, "--junction-file", cohort["index"]] + query)
