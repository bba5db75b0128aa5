"""Pooled samples (`morna supersample`, JunctionStore.pool) without a GPU: the restatement of create_supersample.py of the
reference's tests/ and the numpy restatement of the pool's contract against each other, the two file parsers, the file
writer, what the library refuses before any GPU work, and the command line's argparse errors.  Integers and whole text."""
import gzip

import numpy as np
import pytest

from test_junctions_cpu import sample_lists, store_arrays, tiny_lines


# ---- the restatements --------------------------------------------------------------------------------------------------
def ref_supersample(lines, wanted_ids):
    """create_supersample.py:63-83 line for line on the text lines of an intropolis file (Python 3: a list comprehension
    for izip-free code, str for the gzip bytes); the progress prints left out.  Returns the output file's text."""
    out = []
    for i, line in enumerate(lines):
        coverage = 0
        line_pieces = line.split()
        samples_with_junction = (line_pieces[6].split(','))
        samples_with_junction = [int(num) for num in samples_with_junction]
        samples_junction_coverages = (line_pieces[7].split(','))
        samples_junction_coverages = [int(num) for num in samples_junction_coverages]
        for j, sample in enumerate(samples_with_junction):
            if sample in wanted_ids:
                coverage += samples_junction_coverages[j]
        out.append("\t".join(line_pieces[:3]) + "\t" + str(coverage) + "\n")
    return "".join(out)


def ref_pool(rows, n_lines, group):
    """The contract of morna_jstore_pool for one group: rows[sample] = (line numbers, coverages); group: sample ids, taken
    once each.  Returns (lines int32 ascending, sums int64, holders int32) of the lines at least one member holds."""
    sums, holders = np.zeros(n_lines, np.int64), np.zeros(n_lines, np.int32)
    for s in dict.fromkeys(group):
        line, cov = rows[s]
        np.add.at(sums, np.asarray(line, np.int64), np.asarray(cov, np.int64))
        np.add.at(holders, np.asarray(line, np.int64), 1)
    held = np.nonzero(holders)[0]
    return held.astype(np.int32), sums[held], holders[held]


def rows_of(lines):
    juncs, covrs = sample_lists(lines)
    return {s: (np.array(juncs[s], np.int64), np.array([int(c) for c in covrs[s]], np.int64)) for s in juncs}


def text_from_pool(lines, pooled):
    """The supersample file that follows from a pool's answer: the sum where the line is held, 0 elsewhere."""
    at = dict(zip(pooled[0].tolist(), pooled[1].tolist()))
    return "".join("\t".join(ln.split()[:3]) + "\t" + str(at.get(i, 0)) + "\n" for i, ln in enumerate(lines))


def groups_for(rows):
    ids = list(rows)
    return [[], ids[:1], ids[:5], ids[::3], ids, [ids[0], ids[2], ids[0]], [424242], ids[:4] + [-1, 424242]]


@pytest.mark.parametrize("which", ["tiny", "generic"])
def test_the_two_restatements_agree(which, embedded):
    lines = tiny_lines() if which == "tiny" else embedded["generic"]
    rows = rows_of(lines)
    nonzero = 0
    for group in groups_for(rows):
        known = [s for s in group if s in rows]              # the script sums nothing for an id no line lists
        pooled = ref_pool(rows, len(lines), known)
        text = ref_supersample(lines, group)
        assert text == text_from_pool(lines, pooled)
        assert len(text.splitlines()) == len(lines)
        assert pooled[2].sum() == sum(len(rows[s][0]) for s in set(known))
        nonzero += int(pooled[1].sum() > 0)
    assert nonzero >= 4


def test_ref_pool_keeps_a_held_line_whose_sum_is_zero():
    rows = {1: (np.array([0, 3]), np.array([-7, 2])), 2: (np.array([0]), np.array([7])), 3: (np.array([], np.int64), np.array([], np.int64))}
    lines, sums, holders = ref_pool(rows, 5, [1, 2, 3])
    assert (lines.tolist(), sums.tolist(), holders.tolist()) == ([0, 3], [0, 2], [2, 1])
    assert (lines.dtype, sums.dtype, holders.dtype) == (np.int32, np.int64, np.int32)
    assert [len(x) for x in ref_pool(rows, 5, [3])] == [0, 0, 0]


# ---- the file parsers ----------------------------------------------------------------------------------------------------
def test_parse_sample_ids_file(tmp_path):
    from morna_amd.junctions import parse_sample_ids_file
    p = tmp_path / "ids.txt"
    p.write_text("10223\n\n13224\n  \n14\n-3\n")
    assert parse_sample_ids_file(str(p)) == [10223, 13224, 14, -3]
    p.write_text("")
    assert parse_sample_ids_file(str(p)) == []
    p.write_text("1\n\n2x\n")
    with pytest.raises(ValueError, match="line 3"):
        parse_sample_ids_file(str(p))
    p.write_text("1\n1.5\n")
    with pytest.raises(ValueError, match="line 2"):
        parse_sample_ids_file(str(p))


def test_parse_groups_file(tmp_path):
    from morna_amd.junctions import parse_groups_file
    p = tmp_path / "groups.tsv"
    p.write_text("pancreas\t1,2,3\n\nGTEx_v6.liver-2\t7\nnone\t\nbare\n10\t5,5\n")
    assert parse_groups_file(str(p)) == [("pancreas", [1, 2, 3]), ("GTEx_v6.liver-2", [7]), ("none", []), ("bare", []), ("10", [5, 5])]
    p.write_text("")
    assert parse_groups_file(str(p)) == []
    for text, line in (("a\t1\n\na\t2\n", 3), ("a\t1\nb c\t2\n", 2), ("a\t1\n\n\nb\t1,x\n", 4), ("a\t1\nb\t1,,2\n", 2),
                       ("a\t1.5\n", 1), ("a\t1\t2\n", 1), ("\t1\n", 1), ("a/b\t1\n", 1)):
        p.write_text(text)
        with pytest.raises(ValueError, match="line %d" % line):
            parse_groups_file(str(p))


# ---- the writer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gz", [False, True])
def test_writer_equals_restatement(tmp_path, embedded, gz):
    from morna_amd.junctions import Pooled, write_supersample_files
    for name, lines in (("generic", embedded["generic"]), ("tiny", tiny_lines())):
        src = str(tmp_path / (name + (".gz" if gz else ".tsv")))
        with (gzip.open(src, "wt") if gz else open(src, "w")) as fh:
            fh.write("".join(lines))
        rows = rows_of(lines)
        groups = [g for g in groups_for(rows) if all(s in rows for s in g)]
        jobs = [(str(tmp_path / ("%s.%d" % (name, i))), Pooled(*ref_pool(rows, len(lines), g))) for i, g in enumerate(groups)]
        assert len(jobs) >= 5
        write_supersample_files(src, jobs)
        for (path, _), g in zip(jobs, groups):
            with open(path) as fh:
                assert fh.read() == ref_supersample(lines, g), (name, g)


def test_writer_takes_sums_past_32_bits_and_rejects_a_short_file(tmp_path, embedded):
    from morna_amd.junctions import Pooled, write_supersample_files
    lines = embedded["generic"]
    src = str(tmp_path / "j.tsv")
    with open(src, "w") as fh:
        fh.write("".join(lines))
    big = Pooled(np.array([0, 19], np.int32), np.array([3 * (2**31 - 1), -2**40], np.int64), np.array([3, 1], np.int32))
    write_supersample_files(src, [(str(tmp_path / "big"), big)])
    with open(str(tmp_path / "big")) as fh:
        got = fh.read().splitlines()
    assert len(got) == len(lines) and got[0].split("\t")[3] == "6442450941" and got[19].split("\t")[3] == "-1099511627776"
    assert all(ln.split("\t")[3] == "0" for ln in got[1:19])
    past = Pooled(np.array([len(lines)], np.int32), np.array([1], np.int64), np.array([1], np.int32))
    with pytest.raises(ValueError, match="not the file that was indexed"):
        write_supersample_files(src, [(str(tmp_path / "past"), past)])
    write_supersample_files(src, [])


# ---- what the library refuses, before any GPU work ----------------------------------------------------------------------------
ZERO_STATS = {"kernel_ms": 0.0, "bytes_read": 0, "bytes_written": 0, "workgroups": 0}


def raw_pool(store, members, g_ptr, n_groups=None):
    """morna_jstore_pool itself, past the Python method: (return code, message)."""
    import ctypes as C
    from morna_amd._lib import lib, ptr
    members, g_ptr = np.array(members, np.int64), np.array(g_ptr, np.int64)
    r = C.c_void_p()
    rc = lib().morna_jstore_pool(store._p, ptr(members), ptr(g_ptr), len(g_ptr) - 1 if n_groups is None else n_groups, C.byref(r))
    if rc == 0:
        lib().morna_jpooled_free(r)
    return rc, lib().morna_last_error().decode()


def test_pool_refusals_leave_the_store_usable(embedded):
    import ctypes as C
    from morna_amd import _lib
    from morna_amd.junctions import JunctionStore
    ext, ptr_, line, cov, n_lines = store_arrays(embedded["generic"])
    store = JunctionStore.from_arrays(ext, ptr_, line, cov, n_lines)
    a, b = int(ext[0]), int(ext[1])
    with pytest.raises(IndexError, match="424242"):
        store.pool([[a], [b, 424242]])
    assert store.pool_stats() == ZERO_STATS
    rc, msg = raw_pool(store, [a, b, a, b], [0, 1, 4])                 # a in two groups is allowed; b twice in group 1 is not
    assert rc == _lib.E_INVALID and "group 1" in msg and str(b) in msg and "twice" in msg
    rc, msg = raw_pool(store, [a, b], [1, 2])
    assert rc == _lib.E_INVALID and "start" in msg
    rc, msg = raw_pool(store, [a, b], [0, 2, 1])
    assert rc == _lib.E_INVALID and "descend" in msg and "group 1" in msg
    rc, msg = raw_pool(store, [424242], [0, 1])
    assert rc == _lib.E_RANGE and "424242" in msg
    r = C.c_void_p()
    assert _lib.lib().morna_jstore_pool(store._p, None, None, 1, C.byref(r)) == _lib.E_INVALID
    assert _lib.lib().morna_jstore_pool(store._p, None, _lib.ptr(np.array([0, 1], np.int64)), 1, C.byref(r)) == _lib.E_INVALID
    assert _lib.lib().morna_jstore_pool(None, None, None, 0, C.byref(r)) == _lib.E_INVALID
    assert _lib.lib().morna_jstore_pool(store._p, None, None, 0, None) == _lib.E_INVALID
    assert _lib.lib().morna_jstore_pool_stats(store._p, None) == _lib.E_INVALID
    assert store.pool([]) == [] and store.pool_stats() == ZERO_STATS
    assert raw_pool(store, [], [0], 0)[0] == 0
    assert store.timers()["retain"] == (0.0, 0)
    got_line, got_cov = store.sample(a)                                 # the store still answers
    assert got_line.tolist() == line[ptr_[0]:ptr_[1]].tolist() and got_cov.tolist() == cov[ptr_[0]:ptr_[1]].tolist()


def test_pool_removes_repeats_before_the_library_sees_them(embedded, monkeypatch):
    """JunctionStore.pool hands every id of a group over once, the first time: seen through a stand-in for the call."""
    from morna_amd import junctions
    from morna_amd.junctions import JunctionStore
    ext, ptr_, line, cov, n_lines = store_arrays(embedded["generic"])
    store = JunctionStore.from_arrays(ext, ptr_, line, cov, n_lines)
    seen = {}

    class Stop(Exception):
        pass

    class FakeLib(object):
        def morna_jstore_pool(self, s, members, g_ptr, n, out):
            import ctypes as C
            gp = np.ctypeslib.as_array(C.cast(g_ptr, C.POINTER(C.c_int64)), shape=(n + 1,)).copy()
            seen["g_ptr"] = gp.tolist()
            seen["members"] = np.ctypeslib.as_array(C.cast(members, C.POINTER(C.c_int64)), shape=(int(gp[-1]),)).tolist()
            raise Stop()

    monkeypatch.setattr(junctions, "lib", lambda: FakeLib())
    with pytest.raises(Stop):
        store.pool([[5, 3, 5, 5, 9, 3], [], [3, 3]])
    assert seen == {"g_ptr": [0, 3, 3, 4], "members": [5, 3, 9, 3]}


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from morna_amd import cli
    p = cli.build_parser()
    a = p.parse_args(["supersample", "-x", "idx", "--sample-ids", "ids.txt", "--junction-file", "j.gz", "-o", "out.qry"])
    assert (a.subparser_name, a.basename, a.sample_ids, a.groups, a.junction_file, a.output, a.device) == \
        ("supersample", "idx", "ids.txt", None, "j.gz", "out.qry", "0")
    a = p.parse_args(["supersample", "-x", "idx", "--groups", "g.tsv", "--junction-file", "j.gz", "--output", "out", "--device", "1"])
    assert (a.sample_ids, a.groups, a.output, a.device) == (None, "g.tsv", "out", "1")
    a = p.parse_args(["search", "-x", "idx", "--supersamples", "g.tsv", "--junction-file", "j.gz", "-e", "-d"])
    assert (a.supersamples, a.unhashed_junction_file, a.exact, a.distances) == ("g.tsv", "j.gz", True, True)
    assert p.parse_args(["search", "-x", "idx"]).supersamples is None


SEARCH = ["search", "-x", "idx", "--supersamples", "g.tsv"]


@pytest.mark.parametrize("argv", [
    ["supersample", "-x", "idx", "--junction-file", "j.gz", "-o", "out"],                                  # neither list
    ["supersample", "-x", "idx", "--sample-ids", "i", "--groups", "g", "--junction-file", "j.gz", "-o", "out"],
    ["supersample", "-x", "idx", "--sample-ids", "i", "-o", "out"],                                        # no --junction-file
    ["supersample", "-x", "idx", "--sample-ids", "i", "--junction-file", "j.gz"],                          # no -o
    ["supersample", "--sample-ids", "i", "--junction-file", "j.gz", "-o", "out"],                          # no -x
    SEARCH,                                                                                                 # no --junction-file
    SEARCH + ["--unhashed"],
    SEARCH + ["--junction-file", "j.gz", "-q", "3"],
    SEARCH + ["--junction-file", "j.gz", "--query-ids", "3,4"],
    SEARCH + ["--junction-file", "j.gz", "--intropolis", "q.gz"],
    SEARCH + ["--junction-file", "j.gz", "-c", "10"],
    SEARCH + ["--junction-file", "j.gz", "-rl"],
    SEARCH + ["--junction-file", "j.gz", "--unhashed", "-e"],
    ["junctions", "-x", "idx", "--junction-file", "j.gz", "-sf", "o", "--supersamples", "g.tsv"],
    ["recovery", "-x", "idx", "--supersamples", "g.tsv"],
    ["recovery", "-x", "idx", "-q", "3", "--supersamples", "g.tsv"],
])
def test_parser_errors(argv, capsys):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    assert "supersample" in capsys.readouterr().err
