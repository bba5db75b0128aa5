"""Depth thinning (JunctionStore.thin, --downsample) without a GPU: a numpy restatement of the contract,
its known answers, the properties the contract promises (nesting, independence of the other jobs, unbiasedness), the rate
parser, the --lost-only truth, what the library refuses before any GPU work, the command line's argparse errors, and the
pooled helpers after their refactoring.  Integers and whole text."""
import numpy as np
import pytest

from test_junctions_cpu import store_arrays
from test_pool_cpu import ref_pool, rows_of

GOLDEN_RATIO, KEEP_ALL, MAX_COVERAGE = 0x9e3779b9, 2**32, 2**24
THRESHOLDS = [0, 1, 2**31, 429496730, 2**32 - 1, 2**32]
NESTED = [0, 2**20, 2**31, 3 * 2**30, 2**32]
CHUNK = 2048                                # entries one workgroup of the thin kernels takes
SIZES = [1, 2047, 2048, 2049, 12290]        # line counts of the 200-sample stores
N_SAMPLES, FIRST_ID = 200, 1000
EMPTY, NEGATIVE, TOO_DEEP = 1040, 1190, 1191     # no line; a coverage of -7; a coverage of 2^24 + 1
PLANTED = [0, 1, 31, 32, 33, 64, 65, 4096, 100000]
ROW_LENGTHS = {1041: 1, 1042: 63, 1043: 64, 1044: 65, 1045: CHUNK - 1, 1046: CHUNK, 1047: CHUNK + 1, 1048: 3 * CHUNK + 7}
PLANTED_IN = [1020, 1047, 1048]             # a 5 % row, and the two rows that cross a chunk's edge
DEEPEST = 1048                              # holds the coverage of 2^24, in the largest store only


# ---- the restatement, from the contract ---------------------------------------------------------------------------------------
def fmix32(h):
    """MurmurHash3's finalizer on uint32 arrays (or scalars), modulo 2^32."""
    h = np.array(h, np.uint64) & 0xffffffff
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xffffffff
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xffffffff
    h ^= h >> 16
    return h


def entry_keys(ext, lines, seed):
    """v of every line of sample `ext`."""
    e = int(ext) & (2**64 - 1)
    s = fmix32(int(seed) & 0xffffffff)
    u = fmix32((e & 0xffffffff) ^ int(fmix32((e >> 32) ^ int(s))))
    return fmix32(int(u) ^ (np.asarray(lines, np.int64).astype(np.uint64) & 0xffffffff))


def draws(ext, lines, cov, seed):
    """(h of every draw of every entry as uint64, flat in entry order; the entry every draw belongs to)."""
    cov = np.asarray(cov, np.int64)
    assert len(cov) == 0 or (cov.min() >= 0 and cov.max() <= MAX_COVERAGE), "outside the domain of the contract"
    v = entry_keys(ext, lines, seed)
    entry = np.repeat(np.arange(len(cov)), cov)
    first = np.cumsum(cov) - cov
    i = np.arange(int(cov.sum()), dtype=np.uint64) - np.repeat(first, cov).astype(np.uint64)
    return fmix32((np.repeat(v, cov) + GOLDEN_RATIO * (i + 1)) & 0xffffffff), entry


def kept_of_entry(ext, line, c, a, seed, block=1 << 20):
    """c' of one entry, its draws made `block` at a time: for an entry too deep to lay all its draws out at once."""
    v = int(entry_keys(ext, [line], seed)[0])
    kept = 0
    for first in range(0, int(c), block):
        i = np.arange(first, min(first + block, int(c)), dtype=np.uint64)
        h = fmix32((v + GOLDEN_RATIO * (i + 1)) & 0xffffffff)
        kept += int((h < np.uint64(a)).sum()) if a < KEEP_ALL else len(i)
    return kept


def ref_thin(rows, ext, a, seed, cache=None):
    """The contract of morna_jstore_thin for one job: rows[sample] = (line numbers ascending, coverages); `a` in [0, 2^32].
    Returns (lines int32, thinned coverages int32) of the lines that keep at least one read.  cache: a dict that keeps the
    draws of (ext, seed) between thresholds.  The draws of an entry deeper than 2^20 reads are not laid out with the
    others' but counted in blocks (kept_of_entry), which keeps the temporaries small."""
    lines, cov = np.asarray(rows[ext][0], np.int64), np.asarray(rows[ext][1], np.int64)
    deep = cov > 2**20
    key = (ext, seed)
    if cache is None or key not in cache:
        made = draws(ext, lines, np.where(deep, 0, cov), seed)
        if cache is not None:
            cache[key] = made
    h, entry = cache[key] if cache is not None else made
    kept = np.bincount(entry[h < np.uint64(a)] if a < KEEP_ALL else entry, minlength=len(lines))
    for at in np.nonzero(deep)[0].tolist():
        kept[at] = kept_of_entry(ext, int(lines[at]), int(cov[at]), a, seed)
    on = kept >= 1
    return lines[on].astype(np.int32), kept[on].astype(np.int32)


# ---- the 200-sample stores of the GPU tests, as rows ----------------------------------------------------------------------------
def make_rows(n_lines):
    """200 samples, external ids 1000 .. 1199, over n_lines lines: about 5 % density and coverages 1 + geometric; sample
    1040 empty; rows of exactly 1, 63, 64, 65, chunk - 1, chunk, chunk + 1 and 3 chunk + 7 entries (or every line, where the
    store has fewer); the coverages of PLANTED at the end of three rows; 2^24 in one row of the largest store; one row with a
    coverage of -7 and one with 2^24 + 1, outside the domain."""
    rng = np.random.Generator(np.random.PCG64(20269 + n_lines))
    rows = {}
    for s in range(FIRST_ID, FIRST_ID + N_SAMPLES):
        if s in ROW_LENGTHS:
            line = np.sort(rng.permutation(n_lines)[:min(ROW_LENGTHS[s], n_lines)]).astype(np.int64)
        else:
            line = np.nonzero(rng.random(n_lines) < 0.05)[0].astype(np.int64)
        if s == EMPTY:
            line = line[:0]
        if s in (NEGATIVE, TOO_DEEP, PLANTED_IN[0]) and len(line) == 0:
            line = np.array([n_lines - 1], np.int64)
        cov = rng.geometric(0.2, len(line)).astype(np.int64)
        if s in PLANTED_IN:
            m = min(len(PLANTED), len(cov))
            cov[len(cov) - m:] = PLANTED[:m]
        if s == DEEPEST and n_lines == SIZES[-1]:
            cov[CHUNK] = MAX_COVERAGE                          # the first entry of the row's second chunk
        if s == NEGATIVE:
            cov[len(cov) // 2] = -7
        if s == TOO_DEEP:
            cov[len(cov) // 2] = MAX_COVERAGE + 1
        rows[s] = (line, cov)
    return rows


def good_ids(rows):
    return [s for s in rows if s not in (NEGATIVE, TOO_DEEP)]


@pytest.fixture(scope="module")
def big():
    return make_rows(SIZES[-1])


# ---- the contract ---------------------------------------------------------------------------------------------------------------
def test_known_answers():
    assert int(entry_keys(0, [0], 8675309)[0]) == 0x4b22eeaa
    assert int(entry_keys(1, [7], 8675309)[0]) == 0x9480ee94
    assert int(entry_keys(2**33 + 5, [69999], 8675309)[0]) == 0xad95a227
    h, _ = draws(12, [0], [2], 8675309)
    assert [int(x) for x in h] == [0x1cbbb612, 0xc8ef2bca]
    rows = {12: (np.array([0, 1, 2, 3, 4095, 4096]), np.array([5, 5, 5, 5, 64, 65])),
            21504: (np.array([10, 20, 30]), np.array([1, 1, 100000]))}
    lines, cov = ref_thin(rows, 12, 2**31, 8675309)
    assert (lines.tolist(), cov.tolist()) == ([0, 1, 2, 3, 4095, 4096], [1, 3, 3, 4, 39, 25])
    lines, cov = ref_thin(rows, 21504, 429496730, 1)
    assert (lines.tolist(), cov.tolist()) == ([30], [9845])
    assert (lines.dtype, cov.dtype) == (np.int32, np.int32)


def test_negative_ids_are_their_twos_complement():
    assert int(entry_keys(-1, [3], 5)[0]) == int(entry_keys(2**64 - 1, [3], 5)[0]) != int(entry_keys(2**32 - 1, [3], 5)[0])


def test_nothing_everything_and_nesting(big):
    cache = {}
    for s in (1000, 1020, 1044, 1047, EMPTY):
        lines, cov = big[s]
        got = ref_thin(big, s, 0, 7, cache)
        assert len(got[0]) == 0 and len(got[1]) == 0
        got = ref_thin(big, s, KEEP_ALL, 7, cache)
        assert got[0].tolist() == lines[cov > 0].tolist() and got[1].tolist() == cov[cov > 0].tolist()
        before = np.zeros(SIZES[-1], np.int64)
        for a in NESTED:
            now = np.zeros(SIZES[-1], np.int64)
            got = ref_thin(big, s, a, 7, cache)
            now[got[0]] = got[1]
            assert (now >= before).all(), (s, a)
            before = now
    assert 0 in big[1020][1] and len(ref_thin(big, 1020, KEEP_ALL, 7, cache)[0]) == len(big[1020][0]) - 1   # the planted 0 drops out


def test_a_job_depends_on_its_own_row_only(big):
    alone = {1044: big[1044]}
    moved = {s: big[s] for s in reversed(list(big))}
    for a in (2**31, 429496730):
        want = ref_thin(big, 1044, a, 3)
        for rows in (alone, moved):
            got = ref_thin(rows, 1044, a, 3)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    want = ref_thin(big, 1044, 2**31, 3)                       # but on the seed and on the id it does
    assert ref_thin(big, 1044, 2**31, 4)[1].tolist() != want[1].tolist()
    assert ref_thin({1043: big[1044]}, 1043, 2**31, 3)[1].tolist() != want[1].tolist()


def test_unbiased(big):
    """|kept reads - p C| <= 6 sqrt(C p (1 - p)) for every sample: six sigma of the binomial the contract describes."""
    cache, checked = {}, 0
    for s in good_ids(big):
        C = int(big[s][1].sum())
        for p in (0.01, 0.1, 0.5, 0.9):
            kept = int(ref_thin(big, s, int(round(p * 4294967296.0)), 8675309, cache)[1].sum())
            assert abs(kept - p * C) <= 6 * np.sqrt(C * p * (1 - p)), (s, p, kept, C)
            checked += 1
        cache.clear()
    assert checked == 4 * (N_SAMPLES - 2) and big[DEEPEST][1].max() == MAX_COVERAGE


def test_the_blocked_count_of_a_deep_entry_is_the_flat_one():
    rows = {5: (np.array([3, 9]), np.array([70000, 4])), 6: (np.array([3, 9]), np.array([2**20 + 5, 4]))}
    assert [kept_of_entry(5, 3, 70000, 2**31, 2, block=4096), kept_of_entry(5, 9, 4, 2**31, 2)] == ref_thin(rows, 5, 2**31, 2)[1].tolist()
    h, entry = draws(6, *rows[6], 2)                            # 2^20 + 5 reads: ref_thin takes the blocked way, this the flat one
    assert np.bincount(entry[h < np.uint64(2**31)]).tolist() == ref_thin(rows, 6, 2**31, 2)[1].tolist()
    assert ref_thin(rows, 6, KEEP_ALL, 2)[1].tolist() == [2**20 + 5, 4] and len(ref_thin(rows, 6, 0, 2)[0]) == 0


# ---- the parser and the --lost-only truth -----------------------------------------------------------------------------------------
def test_parse_downsample():
    from morna_amd.junctions import parse_downsample
    assert parse_downsample("0.5,0.1,0.01") == (["0.5", "0.1", "0.01"], [2**31, 429496730, 42949673])
    assert parse_downsample(".1, 1,0,1e-10") == ([".1", "1", "0", "1e-10"], [429496730, 2**32, 0, 0])
    assert parse_downsample("0.75")[1] == [3 * 2**30]
    assert len(parse_downsample(",".join("%.2f" % (i / 16.0) for i in range(16)))[1]) == 16
    for bad in ("", "0.5,", "a", "1/2", "0.5;0.1", "-0.1", "1.0001", "nan", "inf", "0.5,0.50", "1,1.0",
                ",".join("%.3f" % (i / 17.0) for i in range(17))):
        with pytest.raises(ValueError):
            parse_downsample(bad)


def test_lost_lines_on_a_hand_made_row():
    from morna_amd.junctions import lost_lines
    line, cov = [2, 5, 9, 11, 40], [1, 3, 0, 7, 2]
    assert lost_lines(line, cov, [5, 40]).tolist() == [2, 11]              # coverage 0 is never true
    assert lost_lines(line, cov, [5, 40], 2).tolist() == [11]
    assert lost_lines(line, cov, [], 3).tolist() == [5, 11]
    assert lost_lines(line, cov, line).tolist() == [] and lost_lines([], [], []).tolist() == []
    assert lost_lines(line, cov, [5]).dtype == np.int32


# ---- what the library refuses, before any GPU work --------------------------------------------------------------------------------
ZERO_STATS = {"kernel_ms": 0.0, "bytes_read": 0, "bytes_written": 0, "draws": 0, "workgroups": 0}


def raw_thin(store, ext, keep, seed=1, nq=None, null=()):
    """morna_jstore_thin itself, past the Python method: (return code, message)."""
    import ctypes as C
    from morna_amd._lib import lib, ptr
    ext, keep = np.array(ext, np.int64), np.array(keep, np.uint64)
    r = C.c_void_p()
    rc = lib().morna_jstore_thin(None if "store" in null else store._p, None if "ext" in null else ptr(ext),
                                 None if "keep" in null else ptr(keep), len(ext) if nq is None else nq, seed,
                                 None if "out" in null else C.byref(r))
    if rc == 0:
        lib().morna_jthinned_free(r)
    return rc, lib().morna_last_error().decode()


def check_refusals(store, good, negative, too_deep, negative_line, too_deep_line):
    """Every refusal of the contract on `store`; shared with the GPU tests, which then look at the store again."""
    from morna_amd import _lib
    with pytest.raises(IndexError, match="424242"):
        store.thin([good, 424242], 2**31, 1)
    assert store.thin_stats() == ZERO_STATS
    with pytest.raises(ValueError, match=r"%d\D.*line %d\D.*-7" % (negative, negative_line)):
        store.thin([good, negative], 2**31, 1)
    with pytest.raises(ValueError, match=r"%d\D.*line %d\D.*16777217" % (too_deep, too_deep_line)):
        store.thin([too_deep], 0, 1)
    rc, msg = raw_thin(store, [good], [2**32 + 1])
    assert rc == _lib.E_INVALID and "2^32" in msg
    with pytest.raises(ValueError, match="2\\^32"):
        store.thin([good], 2**32 + 1, 1)
    with pytest.raises(ValueError, match="one threshold per job"):
        store.thin([good, good], [1], 1)
    for null in ("store", "ext", "keep", "out"):
        assert raw_thin(store, [good], [1], null=(null,))[0] == _lib.E_INVALID, null
    assert raw_thin(store, [good], [1], nq=-1)[0] == _lib.E_INVALID
    assert _lib.lib().morna_jstore_thin_stats(store._p, None) == _lib.E_INVALID
    assert _lib.lib().morna_jthinned_counts(None, None) == _lib.E_INVALID
    assert _lib.lib().morna_jthinned_job(None, 0, None, None) == _lib.E_INVALID
    assert raw_thin(store, [], [], nq=0, null=("ext", "keep"))[0] == 0
    assert store.thin([], [], 1) == [] and store.thin_stats() == ZERO_STATS


def test_refusals_leave_the_store_usable(embedded):
    from morna_amd.junctions import JunctionStore
    ext, ptr_, line, cov, n_lines = store_arrays(embedded["generic"])
    cov = cov.copy()
    a, b, c = int(ext[0]), int(ext[1]), int(ext[2])
    cov[ptr_[1]] = -7
    cov[ptr_[3] - 1] = 2**24 + 1
    store = JunctionStore.from_arrays(ext, ptr_, line, cov, n_lines)
    check_refusals(store, a, b, c, int(line[ptr_[1]]), int(line[ptr_[3] - 1]))
    assert store.timers()["retain"] == (0.0, 0) and store.pool_stats()["kernel_ms"] == 0.0
    got_line, got_cov = store.sample(a)                                 # the store still answers
    assert got_line.tolist() == line[ptr_[0]:ptr_[1]].tolist() and got_cov.tolist() == cov[ptr_[0]:ptr_[1]].tolist()


def test_rows_without_entries_need_no_gpu():
    from morna_amd.junctions import JunctionStore, Thinned
    store = JunctionStore.from_arrays([5, -6], [0, 0, 0], [], [], 10)
    got = store.thin([5, -6, 5], [0, 2**32, 7], 3)
    assert len(got) == 3 and all(isinstance(r, Thinned) and len(r) == 0 for r in got)
    assert all((r.lines.dtype, r.cov.dtype) == (np.int32, np.int32) for r in got)
    assert store.thin_stats() == ZERO_STATS


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from morna_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["search", "-x", "idx", "--query-ids", "12,34", "--downsample", "0.5,0.1", "--junction-file", "j.gz", "-d", "-e"])
    assert (a.downsample, a.downsample_seed, a.unhashed_junction_file) == ("0.5,0.1", 8675309, "j.gz")
    a = p.parse_args(["recovery", "-x", "idx", "-q", "3", "--downsample", "0.5", "--downsample-seed", "11", "--junction-file", "j.gz",
                      "--lost-only", "--summary-only"])
    assert (a.downsample, a.downsample_seed, a.junction_file, a.lost_only, a.summary_only) == ("0.5", 11, "j.gz", True, True)
    a = p.parse_args(["recovery", "-x", "idx", "-q", "3"])
    assert (a.downsample, a.lost_only) == (None, False)


S = ["search", "-x", "idx", "--downsample", "0.5,0.1"]
R = ["recovery", "-x", "idx", "--downsample", "0.5,0.1"]
JF = ["--junction-file", "j.gz"]


@pytest.mark.parametrize("argv", [
    S + JF,                                                                 # a stream query
    S + JF + ["-f", "bed"],
    S + JF + ["--intropolis", "q.gz"],
    S + JF + ["-q", "3", "--intropolis", "q.gz"],
    S + JF + ["--supersamples", "g.tsv"],
    S + JF + ["-q", "3", "--supersamples", "g.tsv"],
    S + JF + ["-q", "3", "-c", "10"],
    S + JF + ["-q", "3", "-rl"],
    S + ["-q", "3"],                                                        # no --junction-file, not --unhashed
    S + ["--query-ids", "3,4", "-e"],
    R + ["-q", "3"],
    R + JF,
    R + JF + ["--intropolis", "q.gz", "--truth", "t.gz"],
    R + JF + ["-q", "3", "--results-sweep", "5,10"],
    R + JF + ["-q", "3", "-rl"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "-q", "3", "--downsample", "0.5"],
    ["recovery", "-x", "idx", "-q", "3", "--lost-only"],
    ["recovery", "-x", "idx", "-q", "3", "--downsample-seed", "5"],
    ["search", "-x", "idx", "-q", "3", "--downsample-seed", "5"],
    ["search", "-x", "idx", "-q", "3", "--lost-only"],                      # (no such flag in `search`: argparse's own error)
    ["search", "-x", "idx", "-q", "3", "--unhashed", "--downsample", "0.5,x"],
    ["search", "-x", "idx", "-q", "3", "--unhashed", "--downsample", "1.5"],
    ["search", "-x", "idx", "-q", "3", "--unhashed", "--downsample", "0.5,0.5"],
    ["search", "-x", "idx", "-q", "3", "--unhashed", "--downsample", ""],
    ["recovery", "-x", "idx", "-q", "3"] + JF + ["--downsample", ",".join("%.3f" % (i / 17.0) for i in range(17))],
])
def test_parser_errors(argv, capsys):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "downsample" in err or "lost-only" in err


def test_refusals_after_the_parser(tmp_path, monkeypatch):
    """The existing wording: no store next to the index, and one process per shard."""
    from morna_amd import cli
    base = str(tmp_path / "idx")
    commands = [["search", "-x", base, "-q", "3", "--downsample", "0.5", "--junction-file", "j.gz"],
                ["search", "-x", base, "--query-ids", "3,4", "--downsample", "0.5", "--unhashed"],
                ["recovery", "-x", base, "-q", "3", "--downsample", "0.5", "--junction-file", "j.gz"],
                ["recovery", "-x", base, "-q", "3", "--downsample", "0.5", "--junction-file", "j.gz", "--lost-only"]]
    for argv in commands:
        with pytest.raises(IOError, match=r"idx\.junc\.mor not found.*--junction-store"):
            cli.main(argv)
    with open(base + ".shards.mor", "w") as fh:
        fh.write("2\n0 5 10\n")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    for argv in commands:
        with pytest.raises(RuntimeError, match="batch search is not available with one process per shard"):
            cli.main(argv)


def test_recovery_reports_a_job_no_search_answered(monkeypatch, capsys):
    """A job whose search failed as the reference's would is tabulated with no results, named on stderr, and makes the return
    code 1: seen through stand-ins for the search and the store."""
    import io
    from morna_amd import cli
    from morna_amd.junctions import Thinned

    class Store(object):
        def sample(self, ext_id):
            return np.array([1, 4, 6], np.int32), np.array([2, 1, 5], np.int32)

    class Searcher(object):
        internal_id_map = {12: 0, 34: 1}

        def junction_store(self):
            return Store()

        def junction_recovery(self, lists, truth, coverages, truth_min_coverage):
            self.lists, self.truth = lists, [np.asarray(t).tolist() for t in truth]
            return np.zeros((len(lists), 2, 65, len(coverages) + 1), np.int64)

    jobs = [(12, "0.5"), (12, "0"), (34, "0.5"), (34, "0")]
    thinned = [Thinned(np.array([1, 6], np.int32), np.array([1, 2], np.int32)), Thinned(np.zeros(0, np.int32), np.zeros(0, np.int32))] * 2
    results = [([0, 5, 7, 9],), ValueError("math domain error"), ([3, 1, 8],), ([2],)]
    monkeypatch.setattr(cli, "_downsample_search", lambda args, searcher, n, junction_file: (jobs, thinned, results))
    parser = cli.build_parser()
    args = parser.parse_args(["recovery", "-x", "idx", "--query-ids", "12,34", "-r", "2", "--downsample", "0.5,0", "--junction-file", "j.gz",
                              "--lost-only", "--grid", "0:1"])
    cli._check_downsample_flags(parser, args)
    cli._check_recovery_flags(parser, args)
    searcher, out = Searcher(), io.StringIO()
    assert cli._recovery_downsample(args, searcher, out) == 1
    assert capsys.readouterr().err == "query 12 at keep 0 was not searched (math domain error): its table has no results\n"
    assert searcher.lists == [[5, 7], [], [3, 8], [2]]            # the own id removed, the first two kept
    assert searcher.truth == [[4], [1, 4, 6], [4], [1, 4, 6]]     # --lost-only: the lines the thinned row does not hold
    heads = [ln for ln in out.getvalue().splitlines() if ln.startswith("#")]
    assert heads == ["# query 12\tkeep 0.5\tresults 2\ttrue 0", "# query 12\tkeep 0\tresults 0\ttrue 0",
                     "# query 34\tkeep 0.5\tresults 2\ttrue 0", "# query 34\tkeep 0\tresults 1\ttrue 0",
                     "# all 2 queries\tkeep 0.5", "# all 2 queries\tkeep 0"]
    results[1] = ([0],)
    assert cli._recovery_downsample(args, searcher, io.StringIO()) == 0 and capsys.readouterr().err == ""


# ---- the pooled helpers after their refactoring ---------------------------------------------------------------------------------------
def test_pooled_and_thinned_helpers_share_their_code(embedded):
    from morna_amd.junctions import Pooled, Thinned
    from morna_amd.search import MornaSearch
    lines = embedded["generic"]
    rows = rows_of(lines)
    ids = list(rows)
    groups = [ids[:5], ids[::3], [], ids]
    pooled = [Pooled(*ref_pool(rows, len(lines), g)) for g in groups]
    w = np.ones(len(lines), np.float64)
    w[::4] = 0.0
    s = object.__new__(MornaSearch)
    s.unhashed_store = lambda: (None, w)
    handed = []
    s._check_batch_possible = lambda: None
    s._queries_from_rows = lambda rows_, junction_file: handed.append((rows_, junction_file)) or "batch"
    terms = s.unhashed_terms_from_pooled(pooled, ["a", "b", "c", "d"])
    assert len(terms) == 4 and len(terms[2][0]) == 0
    for (l, c), g in zip(terms, groups):
        held, sums, _ = ref_pool(rows, len(lines), g)
        on = w[held] != 0.0
        assert (l.dtype, c.dtype) == (np.int32, np.int32) and l.tolist() == held[on].tolist() and c.tolist() == sums[on].tolist()
    assert 0 < len(terms[3][0]) < len(pooled[3])
    assert s.queries_from_pooled(pooled, ["a", "b", "c", "d"], "j.gz") == "batch"
    assert handed[0][1] == "j.gz" and len(handed[0][0]) == 4
    for (l, c), g in zip(handed[0][0], groups):
        held, sums, _ = ref_pool(rows, len(lines), g)
        assert np.array_equal(l, held) and np.array_equal(c, sums)
    too_big = Pooled(np.array([3], np.int32), np.array([2**31], np.int64), np.array([2], np.int32))
    for call in (lambda: s.queries_from_pooled([too_big], ["big"], "j.gz"), lambda: s.unhashed_terms_from_pooled([too_big], ["big"])):
        with pytest.raises(ValueError, match=r"group big.*line 3"):
            call()
    # a thinned row goes the same way: a sample of its own with the thinned coverages
    longest = max(ids, key=lambda i: len(rows[i][0]))
    thinned = [Thinned(*ref_thin(rows, longest, 2**32 - 1, 5)), Thinned(*ref_thin(rows, ids[1], 0, 5))]
    assert s.queries_from_thinned(thinned, "k.gz") == "batch" and handed[-1][1] == "k.gz"
    assert np.array_equal(handed[-1][0][0][0], thinned[0].lines) and np.array_equal(handed[-1][0][0][1], thinned[0].cov)
    as_pooled = [Pooled(r.lines, r.cov.astype(np.int64), None) for r in thinned]
    got, want = s.unhashed_terms_from_thinned(thinned), s.unhashed_terms_from_pooled(as_pooled, ["x", "y"])
    assert all(a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() for a, b in zip(got, want))
    assert 0 < len(got[0][0]) < len(thinned[0]) and len(got[1][0]) == 0
