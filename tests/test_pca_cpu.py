"""The principal-axes contract without a GPU (include/morna_hip.h, "principal axes"): the numpy restatement
(pca_ref.py) pinned on the summation rule, the start matrix, the sign rule and a matrix whose answer is known in closed form,
its answers against numpy.linalg.eigh, and the host code of `morna pca`: the formatters, the .npz round trip, the parser with
its refusals and the ctypes signatures against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pca_ref import PcaRefused, bs, bs_dot, fix_signs, jacobi, mix, orth, ref_pca, ref_project, start_matrix, unit_rows

U = 2.0 ** -52


# ---- the summation rule ---------------------------------------------------------------------------------------------------

def _terms(n, **at):
    t = np.zeros(n)
    for i, v in at.items():
        t[int(i[1:])] = v
    return t


def test_blocked_sum_order():
    big = 2.0 ** 60
    # +2^60, +1, -2^60 in ascending order lose the 1 wherever a chain or the fold meets it behind 2^60
    assert bs(_terms(600, i0=big, i1=1.0, i2=-big)) == 0.0                             # inside one block
    assert bs(_terms(600, i254=big, i255=1.0, i256=-big)) == 0.0                       # the edge behind the 1
    assert bs(_terms(600, i255=big, i256=1.0, i257=-big)) == 0.0                       # the edge in front of the 1: 1 - 2^60 = -2^60
    assert bs(_terms(600, i0=big, i256=1.0, i512=-big)) == 0.0                         # 256 apart: the fold is ascending too
    assert bs(_terms(600, i0=big, i1=-big, i2=1.0)) == 1.0
    # what one chain over all indices would lose, the blocks keep: 2^53 + 1 + 1 against 2^53 + (1 + 1)
    chain = 0.0
    for v in (2.0 ** 53, 1.0, 1.0):
        chain = chain + v
    assert chain == 2.0 ** 53
    assert bs(_terms(600, i255=2.0 ** 53, i256=1.0, i257=1.0)) == 2.0 ** 53 + 2.0
    assert bs(_terms(600, i254=2.0 ** 53, i255=1.0, i256=1.0)) == 2.0 ** 53            # (both behind 2^53: the first in its chain, the second in the fold)
    # an empty block is added as 0.0; the last block may be ragged; one term
    assert bs(_terms(1000, i999=3.0)) == 3.0 and bs(np.array([5.0])) == 5.0 and bs(np.zeros(0)) == 0.0
    # along an axis, and the dot form
    rng = np.random.default_rng(0)
    A, B = rng.standard_normal((700, 3)), rng.standard_normal((700, 2))
    want = np.array([[bs(A[:, j] * B[:, k]) for k in range(2)] for j in range(3)])
    assert bs_dot(A, B).tobytes() == want.tobytes()
    assert bs(A, axis=0).tobytes() == np.array([bs(A[:, j]) for j in range(3)]).tobytes()
    by_hand = 0.0
    for blk in range(3):
        part = 0.0
        for v in A[256 * blk:256 * blk + 256, 0]:
            part = part + v
        by_hand = by_hand + part
    assert bs(A[:, 0]) == by_hand


def test_start_matrix_against_splitmix64():
    # the published outputs of splitmix64 from the state 0: mix(k * 0x9E3779B97F4A7C15), k = 1, 2, 3
    assert mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert mix((2 * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) == 0x6E789E6AA1B965F4
    assert mix((3 * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) == 0x06C45D188009454F
    assert mix(0) == 0
    G = start_matrix(5, 3, 0)
    assert G[0, 0] == -0.5                                                             # mix(0) = 0
    assert G[1, 2] == float(mix(64 + 2) >> 11) * 2.0 ** -53 - 0.5
    G1 = start_matrix(3, 2, 1)
    assert G1[0, 0] == float(0xE220A8397B1DCDAF >> 11) * 2.0 ** -53 - 0.5
    assert G1[0, 0] == 0x1C4415072F63B9 * 2.0 ** -53 - 0.5                                 # 0xE220A8397B1DCDAF >> 11
    assert start_matrix(3, 2, 2)[0, 0] == float(0x6E789E6AA1B965F4 >> 11) * 2.0 ** -53 - 0.5
    assert G1[2, 1] == float(mix((0x9E3779B97F4A7C15 + 129) & (2 ** 64 - 1)) >> 11) * 2.0 ** -53 - 0.5
    big = start_matrix(400, 8, 7)
    assert big.min() >= -0.5 and big.max() < 0.5 and abs(big.mean()) < 0.02 and len(np.unique(big)) == big.size
    # the seed is taken modulo 2^64
    assert start_matrix(2, 2, 2 ** 64 + 5).tobytes() == start_matrix(2, 2, 5).tobytes()


def test_sign_rule():
    V = np.array([[0.5, -0.5, 0.1], [-0.5, 0.5, -0.7], [0.1, 0.2, 0.7]])
    F = fix_signs(V)
    assert F[:, 0].tolist() == [0.5, -0.5, 0.1]                                        # the tie goes to the lowest z, which is positive
    assert F[:, 1].tolist() == [0.5, -0.5, -0.2]                                       # the lowest z of the tie is negative: negated
    assert F[:, 2].tolist() == [-0.1, 0.7, -0.7]                                       # row 1 (-0.7) comes before row 2 (+0.7)
    assert V[0, 1] == -0.5                                                             # (a copy)


def test_orth_and_jacobi():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((700, 12))
    Q = orth(A)
    assert np.abs(Q.T @ Q - np.eye(12)).max() < 8 * U
    assert np.abs(Q[:, :1] * np.sqrt(bs(A[:, 0] * A[:, 0])) - A[:, :1]).max() < 8 * U
    dep = A.copy()
    dep[:, 5] = 0.0
    with pytest.raises(PcaRefused, match="column 5"):
        orth(dep)
    M = rng.standard_normal((20, 20))
    S = M @ M.T
    S[3, 7] = S[7, 3] = 0.0
    theta, W = jacobi(S)
    lam = np.linalg.eigvalsh(S)[::-1]
    assert np.abs(theta - lam).max() <= 64 * U * lam[0] and (np.diff(theta) <= 0).all()
    assert np.abs(W.T @ W - np.eye(20)).max() < 64 * U and np.abs(S @ W - W * theta[None, :]).max() <= 256 * U * lam[0]
    theta, W = jacobi(np.diag([1.0, 3.0, 3.0, 2.0]))                                   # no rotation; equal values in ascending index
    assert theta.tolist() == [3.0, 3.0, 2.0, 1.0] and W[:, :2].tolist() == np.eye(4)[:, [1, 2]].tolist()


# ---- a matrix whose answer is known -----------------------------------------------------------------------------------------

def _axes_rows(plus1, minus1, plus2, minus2):
    """Rows along +-e1 and +-e2 of 4 columns at power-of-two scales: every unit row is exact."""
    rows = [[2.0 ** (i % 5), 0, 0, 0] for i in range(plus1)] + [[-(2.0 ** (i % 3)), 0, 0, 0] for i in range(minus1)]
    rows += [[0, 0.5, 0, 0]] * plus2 + [[0, -4.0, 0, 0]] * minus2
    return np.array(rows, np.float32)


def test_known_answer_in_closed_form():
    X = _axes_rows(4, 2, 1, 1)
    ok, Ur = unit_rows(X)
    assert ok.all() and set(np.abs(Ur).ravel().tolist()) == {0.0, 1.0}
    # about the origin: the second moments are diag(6/8, 2/8, 0, 0)
    r = ref_pca(X, 2, extra=0, center=False, tol=1e-12, max_iter=50)
    assert r["converged"] and r["fitted"] == 8 and not r["mean"].any() and r["total_variance"] == 1.0
    assert np.abs(r["values"] - [0.75, 0.25]).max() <= 4 * U
    assert np.abs(r["axes"] - np.eye(4)[:2]).max() <= 8 * U
    # about the mean (2/8, 0, 0, 0): the variances are 6/8 - 1/16 and 2/8, the covariance is zero
    r = ref_pca(X, 2, extra=0, center=True, tol=1e-12, max_iter=50)
    assert r["converged"] and r["mean"].tolist() == [0.25, 0.0, 0.0, 0.0]
    assert np.abs(r["values"] - [0.6875, 0.25]).max() <= 4 * U and abs(r["total_variance"] - 0.9375) <= 4 * U
    assert np.abs(r["axes"] - np.eye(4)[:2]).max() <= 8 * U
    coords = ref_project(r["axes"], r["mean"], X.astype(np.float64))
    assert np.abs(coords[0] - [0.75, 0.0]).max() <= 8 * U and np.abs(coords[4] - [-1.25, 0.0]).max() <= 8 * U
    assert np.abs(coords[6] - [-0.25, 1.0]).max() <= 8 * U
    # an allow-list of the e1 rows and one e2 row; a skipped row is left out and gets NaN coordinates
    Xz = np.vstack([X, np.zeros((1, 4), np.float32)])
    allow = np.array([1, 1, 1, 1, 1, 1, 1, 0, 1], bool)
    r = ref_pca(Xz, 1, extra=1, center=False, max_iter=50, allow=allow)
    assert r["fitted"] == 7 and np.abs(r["values"] - [6.0 / 7.0]).max() <= 4 * U
    assert np.isnan(ref_project(r["axes"], r["mean"], Xz.astype(np.float64))[8]).all()
    # rows that are all one unit row e_3: the mean is exact, Z is zero and its first column has no direction
    twins = np.zeros((40, 4), np.float32)
    twins[:, 3] = 2.0
    with pytest.raises(PcaRefused, match="column 0"):
        ref_pca(twins, 2, extra=1, max_iter=2)
    one = ref_pca(twins, 2, extra=1, max_iter=1)                                       # (one iteration orthonormalises the start alone)
    assert one["values"].tolist() == [0.0, 0.0] and one["total_variance"] == 0.0 and one["mean"].tolist() == [0.0, 0.0, 0.0, 1.0]
    for bad in (dict(p=0), dict(p=33), dict(p=2, extra=63), dict(p=2, extra=3), dict(p=1, extra=0, allow=np.arange(8) == 0)):
        with pytest.raises(PcaRefused):
            ref_pca(X, max_iter=2, **bad)


# ---- against numpy.linalg.eigh ----------------------------------------------------------------------------------------------
# The comparison matrix is the fp64 covariance of the same unit rows.  The figures are the restatement's own disagreement with
# eigh on these cases at seed 0, tol 1e-9, extra 8, measured once; a test asserts ten times its figure, the
# margin for the spread between seeds and LAPACK builds, and never more than 1e-7.

def _planted(n, dim, k, seed):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((k, dim)) * 2.0 + 1.0
    lab = rng.integers(0, k, n)
    return (cent[lab] + rng.standard_normal((n, dim))).astype(np.float32)


def _flat(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


CASES = {
    "planted-300x64": (lambda: _planted(300, 64, 5, 1), {2: 2.126e-15, 10: 1.126e-9}, 1.443e-15),
    "planted-700x1100": (lambda: _planted(700, 1100, 6, 2), {2: 5.360e-16, 10: 7.860e-9}, 4.441e-16),
    "planted-400x3000": (lambda: _planted(400, 3000, 4, 3), {2: 6.274e-16, 10: 1.286e-8}, 7.772e-16),
    "flat-300x64": (lambda: _flat(300, 64, 4), {2: 1.212e-9, 10: 1.596e-9}, None),
}
_eigh = {}


def _eigh_of(name):
    if name not in _eigh:
        X = CASES[name][0]()
        _, Ur = unit_rows(X)
        dev = Ur - Ur.mean(axis=0)
        lam, vec = np.linalg.eigh(dev.T @ dev / len(Ur))
        _eigh[name] = (X, lam[::-1], vec[:, ::-1], float(np.trace(dev.T @ dev / len(Ur))))
    return _eigh[name]


@pytest.mark.parametrize("p", [2, 10])
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_eigh(name, p):
    X, lam, vec, trace = _eigh_of(name)
    measured, aligned = CASES[name][1][p], CASES[name][2]
    r = ref_pca(X, p, extra=8, center=True, seed=0, tol=1e-9, max_iter=500)
    assert r["converged"] and r["fitted"] == len(X)
    worst = float(np.max(np.abs(r["values"] - lam[:p])) / lam[0])
    print("%s p=%d: iterations %d, max |theta - lambda| / lambda_0 = %.3e (measured %.3e)" % (name, p, r["iterations"], worst, measured))
    assert worst <= min(10.0 * measured, 1e-7)
    assert abs(r["total_variance"] - trace) <= 1e-12 * trace
    if p == 2 and aligned is not None:
        for j in range(2):
            off = abs(1.0 - abs(float(r["axes"][j] @ vec[:, j])))
            print("%s axis %d: 1 - |v . v_eigh| = %.3e (measured, the larger of the two axes: %.3e)" % (name, j, off, aligned))
            assert off <= 10.0 * aligned
    assert np.abs(r["axes"] @ r["axes"].T - np.eye(p)).max() <= 64 * U


# ---- the host code of `morna pca` -------------------------------------------------------------------------------------------

def test_formatters():
    from morna_amd.search import (SearchPCA, format_pca_components, format_pca_header, format_pca_label_means, format_pca_row,
                                  pca_label_means, pca_shares)
    assert format_pca_header(2, 17, True, 300, 0.5) == "# pca 2\titerations 17\tconverged yes\tsamples 300\ttotal variance 0.5\n"
    assert format_pca_header(1, 500, False, 2, 0.25).split("\t")[2] == "converged no"
    assert pca_shares([0.25, 0.125], 0.5) == [(0.25, 0.5, 0.5), (0.125, 0.25, 0.75)]
    assert format_pca_components([0.25, 0.125], 0.5) == "# pc1\t0.25\t0.5\t0.5\n# pc2\t0.125\t0.25\t0.75\n"
    assert format_pca_components([0.0], 0.0) == "# pc1\t0.0\tnan\tnan\n"
    assert format_pca_row(17, [0.5, -0.25]) == "17\t0.5\t-0.25\n"
    assert format_pca_row(17, [0.5, float("nan")], label="liver", meta="kw") == "17\tliver\t0.5\tnan\tkw\n"
    assert format_pca_row("# query stdin", [1e-30]) == "# query stdin\t1e-30\n"
    assert float(format_pca_row(1, [0.1 + 0.2]).split("\t")[1]) == 0.1 + 0.2           # a coordinate reads back as it was
    coords = np.array([[1.0, 2.0], [3.0, 6.0], [np.nan, np.nan], [5.0, 5.0]])
    means = pca_label_means(["liver", "brain", "gut"], np.array([0, 0, 0, -1], np.int32), coords)
    assert means == [("liver", 2, [2.0, 4.0]), ("brain", 0, None), ("gut", 0, None)]
    assert format_pca_label_means(means) == "# label means\nliver\t2\t2.0\t4.0\nbrain\t0\t-\ngut\t0\t-\n"
    pca = SearchPCA(np.eye(3)[:2], np.zeros(3), np.array([0.25, 0.125]), 4, False, 3, 0.5, None)
    pca.samples, pca.coords = [30, 10, 20], coords[:3]
    assert pca.header() == "# pca 2\titerations 4\tconverged no\tsamples 3\ttotal variance 0.5\n"
    assert pca.components() == format_pca_components([0.25, 0.125], 0.5)
    assert pca.sample_lines() == "30\t1.0\t2.0\n10\t3.0\t6.0\n20\tnan\tnan\n"
    assert pca.sample_lines({30: "liver"}, {10: "kw"}) == "30\tliver\t1.0\t2.0\t-\n10\t-\t3.0\t6.0\tkw\n20\t-\tnan\tnan\t-\n"


def test_axes_file_round_trip(tmp_path):
    from morna_amd.search import SearchPCA, load_pca_axes, save_pca_axes
    rng = np.random.default_rng(5)
    pca = SearchPCA(rng.standard_normal((3, 7)), rng.standard_normal(7), np.array([0.5, 0.25, 0.125]), 12, True, 99, 0.9375, {"t_ms": 1.0})
    path = str(tmp_path / "axes.npz")
    save_pca_axes(path, pca, 7)
    assert os.path.exists(path) and sorted(np.load(path).files) == ["axes", "dim", "info", "mean", "values"]
    back = load_pca_axes(path, 7)
    assert back.axes.tobytes() == pca.axes.tobytes() and back.mean.tobytes() == pca.mean.tobytes()
    assert back.values.tobytes() == pca.values.tobytes() and back.stats is None and back.samples is None
    assert (back.iterations, back.converged, back.fitted, back.total_variance) == (12, True, 99, 0.9375)
    assert back.header() == pca.header() and back.components() == pca.components()
    with pytest.raises(ValueError, match="dimension 7, the index has 8"):
        load_pca_axes(path, 8)
    other = str(tmp_path / "other.npz")
    np.savez(other, mean=pca.mean, axes=pca.axes)
    with pytest.raises(ValueError, match="lacks values, info, dim"):
        load_pca_axes(other, 7)
    np.savez(other, mean=pca.mean[:5], axes=pca.axes, values=pca.values, info=np.zeros(4), dim=np.array(7))
    with pytest.raises(ValueError, match="do not fit"):
        load_pca_axes(other, 7)


def _refused(argv, capsys, text):
    from morna_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert text in err, err


def test_parser_of_its_own():
    from morna_amd import cli
    p = cli.build_pca_parser()
    args = p.parse_args(["-x", "i"])
    assert (args.components, args.extra, args.no_center, args.seed, args.tolerance, args.max_iterations) == (10, 8, False, 0, 1e-9, 500)
    assert (args.within, args.without, args.labels, args.intropolis, args.format, args.save_axes, args.axes, args.output) == (None,) * 8
    assert (args.summary_only, args.metadata, args.device) == (False, False, "0")
    args = p.parse_args(["-x", "i", "-p", "3", "--extra", "5", "--no-center", "--seed", "9", "--tolerance", "1e-6", "--max-iterations", "7",
                         "--within", "w", "--without", "o", "--labels", "l", "--intropolis", "q.gz", "--save-axes", "a.npz", "-o", "c.tsv",
                         "-m", "--device", "1"])
    assert (args.components, args.extra, args.no_center, args.seed, args.tolerance, args.max_iterations) == (3, 5, True, 9, 1e-6, 7)
    assert (args.within, args.without, args.labels, args.intropolis, args.save_axes, args.output, args.metadata, args.device) == \
        ("w", "o", "l", "q.gz", "a.npz", "c.tsv", True, "1")
    assert p.parse_args(["-x", "i", "-f", "bed", "--axes", "a.npz", "--summary-only"]).format == "bed"
    # the pinned parser does not know the word, and is what it was
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["pca", "-x", "i"])
    assert "pca" not in cli._COMMANDS


def test_argparse_errors_before_any_index_is_read(tmp_path, capsys):
    base = ["pca", "-x", "/nonexistent/index"]              # never opened: every case fails in the parser
    ids = tmp_path / "ids.txt"
    ids.write_text("1\n2\n")
    labels = tmp_path / "tissues.tsv"
    labels.write_text("liver\t1,2\nbrain\t3\n")
    _refused(["pca"], capsys, "-x/--basename")
    for p, extra in (("0", "8"), ("33", "0"), ("32", "33"), ("2", "-1"), ("2", "63")):
        _refused(base + ["-p", p, "--extra", extra], capsys, "pca takes 1 to 32 components")
    _refused(base + ["--seed", "-1"], capsys, "--seed takes a number >= 0")
    _refused(base + ["--tolerance", "-1"], capsys, "--tolerance takes a finite number >= 0")
    _refused(base + ["--tolerance", "inf"], capsys, "--tolerance takes a finite number >= 0")
    _refused(base + ["--tolerance", "nan"], capsys, "--tolerance takes a finite number >= 0")
    _refused(base + ["--max-iterations", "0"], capsys, "--max-iterations takes a positive number")
    _refused(base + ["-f", "bam"], capsys, "sam, bed, raw")
    _refused(base + ["-f", "raw", "--intropolis", "q.gz"], capsys, "pca takes one query source")
    _refused(base + ["--summary-only", "-o", "c.tsv"], capsys, "--summary-only and -o cannot be used together")
    for flags, name in ((["-p", "3"], "-p/--components"), (["--extra", "2"], "--extra"), (["--no-center"], "--no-center"),
                        (["--seed", "1"], "--seed"), (["--tolerance", "1e-6"], "--tolerance"), (["--max-iterations", "9"], "--max-iterations"),
                        (["--within", str(ids)], "--within"), (["--without", str(ids)], "--without"), (["--save-axes", "b.npz"], "--save-axes")):
        _refused(base + ["--axes", "a.npz"] + flags, capsys, "--axes cannot be used with %s: the axes are read" % name)
    _refused(base + ["--within", str(ids), "--without", str(ids)], capsys, "--within and --without both name sample id 1")
    _refused(base + ["--within", str(tmp_path / "missing.txt")], capsys, "missing.txt")
    _refused(base + ["--labels", str(tmp_path / "missing.tsv")], capsys, "missing.tsv")
    bad = tmp_path / "bad.tsv"
    bad.write_text("\n")
    _refused(base + ["--labels", str(bad)], capsys, "names no label")
    for flag in (["-r", "5"], ["--search-k", "10"], ["-q", "1"], ["-e"], ["--leave-out-groups", str(labels)], ["-k", "3"]):
        _refused(base + flag, capsys, "unrecognized arguments")
    _refused(base + ["-p", "x"], capsys, "invalid int value")
    # every other command line parses and refuses as before: the word is looked at in the first place only
    _refused(["search", "-x", "i", "pca"], capsys, "unrecognized arguments")
    _refused(["cluster", "-x", "/nonexistent/index"], capsys, "cluster needs -k")


def test_refusals_on_row_shards_and_under_torchrun(tmp_path, monkeypatch):
    from morna_amd import cli
    from morna_amd.search import PCA_SHARDS_REFUSAL, MornaSearch, pca_width_refusal
    base = str(tmp_path / "idx")
    open(base + ".shards.mor", "w").close()
    with pytest.raises(SystemExit):
        cli.main(["pca", "-x", base])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cli.main(["pca", "-x", str(tmp_path / "plain")])
    monkeypatch.delenv("WORLD_SIZE")
    assert "row shards" in PCA_SHARDS_REFUSAL
    s = MornaSearch.__new__(MornaSearch)
    s.annoy_index = object()                    # stands for shards.LocalShards: not one AnnoyIndex
    with pytest.raises(ValueError) as e:
        s.principal_axes(2)
    assert str(e.value) == PCA_SHARDS_REFUSAL
    with pytest.raises(ValueError) as e:
        s.pca_coordinates(None, [0])
    assert str(e.value) == PCA_SHARDS_REFUSAL
    assert "-p 40 --extra 8" in pca_width_refusal(40, 8)


# ---- the ctypes table against the header's prototypes ----------------------------------------------------------------------

def _ctype_of(decl):
    decl = re.sub(r"\bconst\b", "", decl).strip()
    stars = decl.count("*")
    base = decl.replace("*", " ").split()[0]
    if stars == 2:
        return C.POINTER(C.c_void_p)
    if stars == 1:
        return C.c_void_p
    return {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int,
            "double": C.c_double}[base]


def test_ctypes_signatures_match_the_header():
    from morna_amd import _lib
    from morna_amd.annoy import PCA_STATS
    from morna_amd.search import PCA_MAX_BLOCK, PCA_MAX_COMPONENTS
    with open(os.path.join(ROOT, "include", "morna_hip.h")) as fh:
        src = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in ("morna_pca", "morna_pca_project", "morna_pca_stats"):
        m = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, name
        res, args = _lib.SIGNATURES[name]
        assert res is _ctype_of(m.group(1)), name
        want = [_ctype_of(a) for a in m.group(2).split(",")]
        assert len(args) == len(want), name
        for i, (got, w) in enumerate(zip(args, want)):
            assert got is w, (name, i, got, w)
    m = re.search(r"morna_pca\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "r", "p", "extra", "center", "seed", "tol", "max_iter", "axes_out", "mean_out", "values_out", "info_out"]
    m = re.search(r"morna_pca_project\s*\(([^)]*)\)", src)
    names = [a.replace("*", " ").split()[-1] for a in m.group(1).split(",")]
    assert names == ["h", "axes", "mean", "p", "q", "items", "nq", "coords_out"]
    assert re.search(r"#define\s+MORNA_PCA_MAX_COMPONENTS\s+%d\b" % PCA_MAX_COMPONENTS, src)
    assert re.search(r"#define\s+MORNA_PCA_MAX_BLOCK\s+%d\b" % PCA_MAX_BLOCK, src)
    assert len(PCA_STATS) == 8
