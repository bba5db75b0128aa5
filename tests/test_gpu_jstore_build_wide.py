"""`JunctionStore.build` on both sides of the count kernel's LDS bitmap: files of 262144 samples, the last the bitmap of 2 x
8192 words holds, and of 262145, where the host looks for a sample a line lists twice and the kernel runs without the
bitmap.  The built store, as the bytes it saves, against a numpy stable sort of the file's entries by sample
(jstore_big.expected_store, which test_jstore_big_cpu.py pins to the dict-and-list restatement on the embedded files); and
what both paths refuse, in the same words.

The files are parsed from gzip text: a ParsedLines.from_arrays parse records no count of lines read, so jstore_build's guard
against a parse that dropped lines ("a whole parse with threshold 0") refuses it.  Text has no line without entries, so
there is none here.  40 lines are three of the build's blocks of 16, the last of 8; the line of all samples is in the second
(512 strides of the kernel's threads beside a count table of three blocks), and 262145 samples are 257 per thread of
jstore_ptr_kernel.  Integers and whole files; no tolerance.  -m gpu"""
import numpy as np
import pytest

import jstore_big as big

pytestmark = pytest.mark.gpu


def parsed(path, samples, covs):
    from morna_amd.index import ParsedLines
    big.write_lines(path, samples, covs)
    return ParsedLines(path, sample_count=1, sample_threshold=0)


@pytest.fixture(scope="module", params=big.WIDE_SIZES)
def wide(request, tmp_path_factory):
    S = request.param
    d = tmp_path_factory.mktemp("wide%d" % S)
    samples, covs = big.wide_lines(S)
    lines = parsed(str(d / "good.tsv.gz"), samples, covs)
    assert (lines.n_lines, lines.lines_read, lines.n_items, lines.nnz) == (big.WIDE_J, big.WIDE_J, S, sum(len(x) for x in samples))
    ext, ptr, line, cov = big.expected_store(samples, covs)
    return dict(S=S, dir=d, samples=samples, covs=covs, lines=lines, ext=ext, ptr=ptr, line=line, cov=cov,
                blob=big.store_file_bytes(ext, ptr, line, cov, big.WIDE_J))


def saved(store, path):
    store.save(str(path))
    with open(str(path), "rb") as fh:
        return fh.read()


def build_and_compare(wide, name):
    from morna_amd.junctions import JunctionStore
    store = JunctionStore.build(wide["lines"])
    assert (store.n_samples, store.nnz, store.n_lines) == (wide["S"], len(wide["line"]), big.WIDE_J)
    assert saved(store, wide["dir"] / name) == wide["blob"]
    return store


def test_built_store_equals_the_stable_sort(wide):
    S, ext, ptr, line, cov = wide["S"], wide["ext"], wide["ptr"], wide["line"], wide["cov"]
    store = build_and_compare(wide, "first.junc.mor")
    assert store.sample_ids().tobytes() == ext.tobytes()
    rng = np.random.Generator(np.random.PCG64(S))
    edge = [0, 1, 31, 32, S - 33, S - 32, S - 31, S - 2, S - 1]               # internal ids: the samples of the edge line and their neighbours
    for s in edge + rng.choice(S, 300, replace=False).tolist():
        got_line, got_cov = store.sample(int(ext[s]))
        assert got_line.tobytes() == line[ptr[s]:ptr[s + 1]].tobytes() and got_cov.tobytes() == cov[ptr[s]:ptr[s + 1]].tobytes(), s
    for s, c in ((S - 1, big.BIG), (S - 32, 0), (S - 33, -5), (0, -2**31)):    # the edge line's entries and their coverages
        got_line, got_cov = store.sample(int(ext[s]))
        assert got_cov[got_line == big.EDGE_LINE].tolist() == [c] and big.ALL_LINE in got_line.tolist(), s
    assert store.timers()["build"][0] > 0 and store.timers()["build"][1] == 16 * store.nnz
    again = build_and_compare(wide, "second.junc.mor")         # two builds of the same lines: the same bytes
    assert again.sample_ids().tobytes() == ext.tobytes()


def refused(wide, name, changes, message):
    """The file with the lines of `changes` ({line: (samples, covs)}) put in is refused with `message`; the good lines then
    build, in the same process, to the same bytes."""
    from morna_amd.junctions import JunctionStore
    samples, covs = list(wide["samples"]), list(wide["covs"])
    for j, (ids, c) in changes.items():
        samples[j], covs[j] = ids, c
    bad = parsed(str(wide["dir"] / (name + ".tsv.gz")), samples, covs)
    assert (bad.n_lines, bad.n_items) == (big.WIDE_J, wide["S"])
    with pytest.raises(ValueError) as e:
        JunctionStore.build(bad)
    assert message in str(e.value), str(e.value)
    build_and_compare(wide, name + ".junc.mor")


def test_a_repeat_of_the_last_sample_is_refused(wide):
    S, ext, samples, covs = wide["S"], wide["ext"], wide["samples"], wide["covs"]
    last = int(ext[S - 1])                                     # the last bit of the bitmap's last word at 262144 samples
    refused(wide, "once", {33: big.with_repeat(samples[33], covs[33], last)}, "line 33 lists sample %d twice" % last)


def test_the_earliest_line_of_two_that_repeat_is_named(wide):
    S, ext, samples, covs = wide["S"], wide["ext"], wide["samples"], wide["covs"]
    last, other = int(ext[S - 1]), int(ext[7])
    refused(wide, "two_lines", {33: big.with_repeat(samples[33], covs[33], last), 35: big.with_repeat(samples[35], covs[35], other)},
            "line 33 lists sample %d twice" % last)


def test_the_smallest_sample_of_two_a_line_repeats_is_named(wide):
    """One line lists two samples twice each, the one of the larger internal id first.  The count kernel reports the smallest
    (line, internal id); the host's loop past the bitmap must name the same sample, not the first repeat it meets."""
    S, ext, samples, covs = wide["S"], wide["ext"], wide["samples"], wide["covs"]
    low, high = int(ext[5]), int(ext[S - 2])
    keep = ~np.isin(samples[34], [low, high])
    ids = np.concatenate([samples[34][keep], [high, high, low, low]])
    c = np.concatenate([covs[34][keep], [4, 4, 6, 6]])
    refused(wide, "two_samples", {34: (ids, c)}, "line 34 lists sample %d twice" % low)


def test_a_sample_past_the_last_is_refused_before_the_build(wide):
    """An entry that names sample S never reaches jstore_count_kernel's range counter: text gives every id it meets a
    sample of its own, and lines_from_arrays refuses an item id outside [0, S).  That refusal is what is pinned here; the
    kernel's counter stays unexercised."""
    from morna_amd.index import ParsedLines
    S = wide["S"]
    prep = dict(key_bytes=np.frombuffer(b"chr1 1 2", np.uint8), key_off=np.array([0, 8], np.int64), row_ptr=np.array([0, 3], np.int64),
                ids=np.array([0, S - 1, S], np.int32), cov=np.array([1, 2, 3], np.int32), idf=np.zeros(1), ext_ids=np.arange(S, dtype=np.int64))
    with pytest.raises(IndexError, match=r"item id %d out of range \[0, %d\)" % (S, S)):
        ParsedLines.from_arrays(prep, S)
    prep["ids"] = np.array([0, S - 1, S - 2], np.int32)
    assert ParsedLines.from_arrays(prep, S).n_items == S
    build_and_compare(wide, "after_range.junc.mor")
