"""The recovery sweep on the GPU: one histogram per prefix length of every result list from one pass.
Slice [q][i] against the numpy restatement (test_recovery_cpu.ref_hist) of the list cut to p_i results and against the
shipped one-length kernel fed that cut list, entry for entry; the statistics, the refusals and the command line.
Integers and whole text only, no tolerance.  -m gpu"""
import re

import numpy as np
import pytest

from test_gpu_junctions import _write_gz, blocks, result_ids, run_cli
from test_gpu_recovery import EMPTY, GRID8, GRID15, make_store, summary_text, table_text, truth_of_sample
from test_junctions_cpu import sample_lists
from test_recovery_cpu import ref_hist, rows_of_tables

pytestmark = pytest.mark.gpu

# Bucket sizes 1, 2, 2, 1, 15, 41, 1, 1: not multiples of the four waves, and single ranks; 3 and 5 fall between the repeats
# of 1003 in make_store's list 6 (ranks 0, 2, 5); most lie beyond the end of lists 0-3, 6 and 7; 64 is the whole word.
PREFIXES = [1, 3, 5, 6, 21, 62, 63, 64]
SIZES = [1, 4097, 12290]                   # one tile, just past a tile edge, three tiles and a remainder
# make_store's eight lists and one more: 1000 alone holds line 0 with the store's one negative coverage, then the empty
# sample, then 1007 and 1014, which hold line 0 too (every seventh sample does), with coverages of 1 or more
JOINED = [1000, EMPTY, 1007, 1003, 1014, 1021, 1002]
TRUTH_IDS = [1000, 1000, EMPTY, 1005, 1095, 1014, 1003, 1021, 1007]


@pytest.fixture(scope="module", params=SIZES)
def case(request):
    c = make_store(request.param)
    c["lists"] = c["lists"] + [JOINED]
    c["want"] = {}
    return c


def cut(lists, p):
    return [lst[:p] for lst in lists]


def want(case, min_cov, grid_name):
    """ref_hist of every list cut to every prefix, [nq][P][2][65][B + 1]; made once per (truth coverage, grid)."""
    key = (min_cov, grid_name)
    if key not in case["want"]:
        grid = {"GRID8": GRID8, "GRID15": GRID15}[grid_name]
        truths = [truth_of_sample(case, s, min_cov) for s in TRUTH_IDS]
        case["want"][key] = np.stack([np.stack([ref_hist(case["rows"], case["n_lines"], lst[:p], t, grid) for p in PREFIXES])
                                      for lst, t in zip(case["lists"], truths)])
    return case["want"][key]


def classes(case, lst, grid):
    """(cnt, b) of every line under one list, as ref_hist classifies them."""
    n = case["n_lines"]
    cnt, mx = np.zeros(n, np.int64), np.full(n, -2**31, np.int64)
    for s in lst:
        line, cov = case["rows"][s]
        cnt[line] += 1
        mx[line] = np.maximum(mx[line], cov)
    return cnt, np.where(cnt > 0, np.searchsorted(np.asarray(grid, np.int64), mx, side="right"), 0)


def entries(case, samples):
    return sum(len(case["rows"][s][0]) for s in samples)


# ---- the slices ----------------------------------------------------------------------------------------------------------
def test_the_running_maximum_is_exercised(case):
    """The oracle itself, no library call: between consecutive prefixes some line that was already held reaches more
    thresholds, because a larger coverage arrives in a later bucket; and line 0, held first by 1000 alone at coverage -7
    (one threshold of GRID15), reaches more once 1007 joins.  Without both, a kernel that classified every prefix from
    the first bucket's maxima would pass the comparisons below."""
    before_cnt, before_b = classes(case, JOINED[:1], GRID15)
    after_cnt, after_b = classes(case, JOINED[:3], GRID15)
    assert (before_cnt[0], before_b[0]) == (1, 1) and after_cnt[0] == 2 and after_b[0] >= 3
    risen = 0
    for lst in case["lists"]:
        for p, p_next in zip(PREFIXES, PREFIXES[1:]):
            (cnt, b), (_, b_next) = classes(case, lst[:p], GRID15), classes(case, lst[:p_next], GRID15)
            risen += int(((cnt > 0) & (b_next > b)).sum())
    assert risen > 0
    # and the truths put line 0 of JOINED on plane 1, where the histogram shows it: 1007 covers line 0 at least once
    assert 0 in truth_of_sample(case, TRUTH_IDS[8], 1).tolist()


@pytest.mark.parametrize("form", ["sample", "lines"])
@pytest.mark.parametrize("min_cov", [1, 3])
def test_slices_equal_restatement_and_shipped_kernel(case, form, min_cov):
    store, lists = case["store"], case["lists"]
    truths = [truth_of_sample(case, s, min_cov) for s in TRUTH_IDS]
    if form == "sample":
        got = store.recovery_sweep_by_sample(lists, TRUTH_IDS, GRID15, PREFIXES, truth_min_coverage=min_cov)
    else:
        got = store.recovery_sweep(lists, truths, GRID15, PREFIXES)
    assert got.dtype == np.int64 and got.shape == (len(lists), len(PREFIXES), 2, 65, 16)
    expected = want(case, min_cov, "GRID15")
    for i, p in enumerate(PREFIXES):
        assert np.array_equal(got[:, i], expected[:, i]), p
        shipped = store.recovery_by_sample(cut(lists, p), TRUTH_IDS, GRID15, truth_min_coverage=min_cov)
        assert np.array_equal(got[:, i], shipped), p
    assert got[:, :, 0, 0].sum() == 0
    for q, lst in enumerate(lists):                            # prefixes that clamp to one length: one array
        for i, p in enumerate(PREFIXES):
            for j in range(i + 1, len(PREFIXES)):
                if min(p, len(lst)) == min(PREFIXES[j], len(lst)):
                    assert np.array_equal(got[q, i], got[q, j]), (q, p, PREFIXES[j])
    missed = got[0, :, 1, 0, 0]                                # the empty list: every true line missed, under every prefix
    assert (missed == len(truths[0])).all() and got[0].sum() == missed.sum()
    # line 0 of JOINED: at prefix 1 held once, one threshold reached (-7); at prefix 3 held twice and more reached
    t0 = int(0 in truths[8].tolist())
    assert got[8, 0, t0, 1, 1] >= 1 and got[8, 1, t0, 1, 1] == got[8, 0, t0, 1, 1] - 1
    if case["n_lines"] == 1:                                   # the file IS line 0: the slice shows its class alone
        assert got[8, 0].sum() == 1 and got[8, 1].sum() == 1 and got[8, 1, t0, 2, 3:].sum() == 1


def test_one_prefix_is_the_old_call(case):
    store, lists = case["store"], case["lists"]
    whole = store.recovery_sweep_by_sample(lists, TRUTH_IDS, GRID8, [64])
    assert whole.shape == (len(lists), 1, 2, 65, 9)
    assert np.array_equal(whole[:, 0], store.recovery_by_sample(lists, TRUTH_IDS, GRID8))
    assert np.array_equal(whole[:, 0], want(case, 1, "GRID8")[:, 7])
    twenty = store.recovery_sweep_by_sample(lists, TRUTH_IDS, GRID8, [20])
    assert np.array_equal(twenty[:, 0], store.recovery_by_sample(cut(lists, 20), TRUTH_IDS, GRID8))


def test_slices_do_not_depend_on_the_batch(case):
    store = case["store"]
    lst, other = case["lists"][3], case["lists"][5]
    one = store.recovery_sweep_by_sample([lst], [1005], GRID8, [5, 20])
    three = store.recovery_sweep_by_sample([other, lst, []], [1001, 1005, 1005], GRID8, [5, 20])
    many = store.recovery_sweep_by_sample([lst] * 64 + [other], [1005] * 64 + [1001], GRID8, [5, 20])
    assert np.array_equal(one[0], three[1]) and np.array_equal(three[0], many[64])
    assert all(np.array_equal(one[0], many[q]) for q in range(64))
    for i, p in enumerate([5, 20]):
        assert np.array_equal(one[0, i], ref_hist(case["rows"], case["n_lines"], lst[:p], truth_of_sample(case, 1005, 1), GRID8))
    assert not np.array_equal(one[0, 0], one[0, 1]) or case["n_lines"] == 1


def test_stats_count_the_rows_once(case):
    store, lists = case["store"], case["lists"]
    n_tiles = (case["n_lines"] + 4095) // 4096
    prefixes = [2, 5, 21]                                      # the last cuts lists 4 and 5 (63 and 64 results) to 21 rows
    read = [s for lst in lists for s in lst[:21]]
    store.recovery_sweep_by_sample(lists, TRUTH_IDS, GRID8, prefixes)
    stats = store.recovery_stats()
    assert stats["bytes"] == 8 * (entries(case, read) + entries(case, TRUTH_IDS))
    assert stats["workgroups"] == len(lists) * n_tiles and stats["kernel_ms"] > 0
    truths = [truth_of_sample(case, s, 1) for s in TRUTH_IDS]
    store.recovery_sweep(lists, truths, GRID8, prefixes)
    stats = store.recovery_stats()
    assert stats["bytes"] == 8 * entries(case, read) + 4 * sum(len(t) for t in truths)
    assert stats["workgroups"] == len(lists) * n_tiles and stats["kernel_ms"] > 0
    store.recovery_by_sample(lists, TRUTH_IDS, GRID8)          # the statistics are the last call's, of either kind
    assert store.recovery_stats()["bytes"] == 8 * (entries(case, [s for lst in lists for s in lst]) + entries(case, TRUTH_IDS))
    for empty in (store.recovery_sweep([], [], GRID8, prefixes), store.recovery_sweep_by_sample([], [], GRID8, prefixes)):
        assert empty.shape == (0, 3, 2, 65, 9) and empty.dtype == np.int64
        assert store.recovery_stats() == {"kernel_ms": 0.0, "bytes": 0, "workgroups": 0}


# ---- refusals ------------------------------------------------------------------------------------------------------------
def raw_sweep(store, lists, truth_ids, grid, prefixes, null_prefixes=False):
    """morna_jstore_recovery_sweep_by_sample itself: (return code, message, hist)."""
    from morna_amd._lib import lib, ptr
    k = max([len(lst) for lst in lists] + [1])
    res = np.zeros((len(lists), k), np.int64)
    n_res = np.array([len(lst) for lst in lists], np.int32)
    for q, lst in enumerate(lists):
        res[q, :len(lst)] = lst
    truth, grid, pre = np.array(truth_ids, np.int64), np.array(grid, np.int64), np.array(prefixes, np.int32)
    hist = np.zeros((len(lists), 8, 2, 65, len(grid) + 1), np.int32)
    rc = lib().morna_jstore_recovery_sweep_by_sample(store._p, ptr(res), ptr(n_res), len(lists), k, ptr(truth), 1, ptr(grid), len(grid),
                                                     None if null_prefixes else ptr(pre), len(pre), ptr(hist))
    return rc, lib().morna_last_error().decode(), hist


def test_refusals_leave_the_store_usable():
    from morna_amd._lib import E_INVALID
    case = make_store(4097)
    store, lst = case["store"], case["lists"][3]
    truth = truth_of_sample(case, 1005, 1)
    good = np.stack([ref_hist(case["rows"], 4097, lst[:p], truth, GRID8) for p in (5, 20)])[None]

    def still_works():
        assert np.array_equal(store.recovery_sweep([lst], [truth], GRID8, [5, 20]), good)
        assert np.array_equal(store.recovery_sweep_by_sample([lst], [1005], GRID8, [5, 20]), good)
    still_works()
    for prefixes, named in (([], ["0"]), (list(range(1, 10)), ["9"]), ([0], ["0"]), ([65], ["65"]), ([5, 5], ["5", "ascend"]),
                            ([10, 5], ["10", "5", "ascend"]), ([3, -2], ["-2"])):
        rc, message, hist = raw_sweep(store, [lst], [1005], GRID8, prefixes)
        assert rc == E_INVALID and all(word in message for word in named), (prefixes, message)
        assert hist.sum() == 0
        with pytest.raises(ValueError):
            store.recovery_sweep_by_sample([lst], [1005], GRID8, prefixes)
        with pytest.raises(ValueError):
            store.recovery_sweep([lst], [truth], GRID8, prefixes)
        still_works()
    rc, message, hist = raw_sweep(store, [lst], [1005], GRID8, [5, 20], null_prefixes=True)
    assert rc == E_INVALID and "prefixes" in message and hist.sum() == 0
    still_works()
    # what the one-length call refuses, the sweep refuses in its words
    with pytest.raises(ValueError, match="ascend"):
        store.recovery_sweep_by_sample([lst], [1005], [10, 5], [5, 20])
    with pytest.raises(IndexError, match="424242"):
        store.recovery_sweep_by_sample([[1000, 424242]], [1005], GRID8, [1])
    with pytest.raises(IndexError, match="515151"):
        store.recovery_sweep_by_sample([lst], [515151], GRID8, [5, 20])
    with pytest.raises(ValueError, match="position 1 of list 0"):
        store.recovery_sweep([lst], [[7, 3]], GRID8, [5, 20])
    with pytest.raises(ValueError, match="one truth per result list"):
        store.recovery_sweep_by_sample([lst, lst], [1005], GRID8, [5, 20])
    still_works()
    rc, message, hist = raw_sweep(store, [lst], [1005], GRID8, [5, 20])                  # and the raw call agrees when all is well
    assert rc == 0 and np.array_equal(hist[:, :2].astype(np.int64), good)


# ---- the command line on the embedded fixture ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def generic(tmp_path_factory, embedded):
    d = tmp_path_factory.mktemp("recovery_sweep_generic")
    src, base = str(d / "junctions.gz"), str(d / "idx")
    _write_gz(src, embedded["generic"])
    rc, _, _ = run_cli(["index", "--intropolis", src, "-x", base, "--features", "128", "--n-trees", "5", "-s", "10", "-t", "4",
                        "--junction-store"])
    assert rc == 0
    return dict(base=base, lines=embedded["generic"], tables=sample_lists(embedded["generic"]))


def headed_blocks(text):
    """[(header line, the lines under it)] of a `recovery` output."""
    parts = re.split(r"^(# .*\n)", text, flags=re.M)
    assert parts[0] == ""
    return [(parts[i], parts[i + 1]) for i in range(1, len(parts), 2)]


def test_command_line_sweep_equals_separate_runs(generic):
    ids, depth, sweep = [3, 7, 10], 8, [2, 5, 8]               # ten samples: a query has nine others
    flags = ["recovery", "-x", generic["base"], "-e", "--query-ids", ",".join(map(str, ids))]
    rc, out, _ = run_cli(flags + ["-r", str(depth), "--results-sweep", "8,2,5"])
    assert rc == 0
    got = headed_blocks(out)
    assert [h for h, _ in got[:9]] == ["# query %d\tresults %d\ttrue %d\n" % (q, p, len(generic["tables"][0][q]))
                                       for q in ids for p in sweep]
    assert [h for h, _ in got[9:]] == ["# all 3 queries\tresults %d\n" % p for p in sweep]
    for i, p in enumerate(sweep):
        rc, alone, _ = run_cli(flags + ["-r", str(p)])
        assert rc == 0
        separate = headed_blocks(alone)
        assert len(separate) == 4 and separate[3][0] == "# all 3 queries\n"
        for j in range(3):
            assert got[3 * j + i] == separate[j], (p, ids[j])  # header and table, byte for byte
        assert got[9 + i][1] == separate[3][1], p
    assert len(set(body for _, body in got[9:])) == 3          # the result count matters on this fixture
    rc, only, _ = run_cli(flags + ["-r", str(depth), "--results-sweep", "8,2,5", "--summary-only"])
    assert rc == 0 and only == "".join(h + body for h, body in got[9:])
    with pytest.raises(SystemExit) as e:                       # a count past -r never reaches the index
        run_cli(flags + ["-r", "5", "--results-sweep", "2,8"])
    assert e.value.code == 2


def test_command_line_without_the_sweep_is_unchanged(generic):
    from morna_amd.junctions import parse_recovery_grid
    from morna_amd.search import MornaSearch
    frequencies, coverages = parse_recovery_grid()
    inv = {v: k for k, v in MornaSearch(generic["base"]).internal_id_map.items()}
    rows_by_sample = rows_of_tables(generic["tables"])
    ids = [3, 7, 10]
    flags = ["-x", generic["base"], "-e", "--query-ids", ",".join(map(str, ids))]
    rc, out, _ = run_cli(["recovery", "-r", "8"] + flags)
    assert rc == 0
    _, searched, _ = run_cli(["search", "-r", "9"] + flags)
    texts, tables = [], []
    for q, body in blocks(searched):
        results = [inv[i] for i in result_ids(body) if inv[i] != q][:8]
        assert len(results) == 8
        text, rows = table_text(rows_by_sample, len(generic["lines"]), q, results, generic["tables"][0][q], 0, frequencies, coverages)
        texts.append(text)
        tables.append(rows)
    assert len(texts) == 3 and out == "".join(texts) + summary_text(tables)
    rc, only, _ = run_cli(["recovery", "-r", "8", "--summary-only"] + flags)
    assert rc == 0 and only == summary_text(tables)
