"""`morna pca` on the command line, on the 600-sample cohort of test_gpu_restrict_cli.py: the whole text
against the restatement (pca_ref.py) and the formatters, --within with every sample still listed, the --labels block,
--save-axes and --axes, the "# query" lines of --intropolis and of a stream, and `search` and `cluster` left as they were.
-m gpu"""
import numpy as np
import pytest

from pca_ref import ref_pca, ref_project
from test_gpu_junctions import run_cli
from test_gpu_restrict_cli import N_INDEX, cohort  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def searcher(cohort):  # noqa: F811
    from morna_amd.search import MornaSearch
    return MornaSearch(cohort["base"])


@pytest.fixture(scope="module")
def rows(searcher):
    return searcher.annoy_index.get_items()


def header_text(want, p):
    out = ["# pca %d\titerations %d\tconverged %s\tsamples %d\ttotal variance %s\n"
           % (p, want["iterations"], "yes" if want["converged"] else "no", want["fitted"], want["total_variance"])]
    running = 0.0
    for j, v in enumerate(want["values"].tolist()):
        running += v / want["total_variance"]
        out.append("# pc%d\t%s\t%s\t%s\n" % (j + 1, v, v / want["total_variance"], running))
    return "".join(out)


def sample_text(cohort, coords, labels=None):  # noqa: F811
    inv = cohort["inv"]
    return "".join("\t".join([str(inv[i])] + ([labels.get(inv[i], "-")] if labels is not None else []) + [str(c) for c in row]) + "\n"
                   for i, row in enumerate(coords.tolist()))


def test_whole_text(cohort, searcher, rows):  # noqa: F811
    want = ref_pca(rows, 3, extra=5, tol=1e-9, max_iter=500)
    assert want["converged"] and want["fitted"] == N_INDEX
    coords = ref_project(want["axes"], want["mean"], rows.astype(np.float64))
    argv = ["pca", "-x", cohort["base"], "-p", "3", "--extra", "5"]
    rc, text, _ = run_cli(argv)
    assert rc == 0 and text == header_text(want, 3) + sample_text(cohort, coords)
    rc, text, _ = run_cli(argv + ["--summary-only"])
    assert rc == 0 and text == header_text(want, 3)
    out_file = str(cohort["dir"] / "coords.tsv")
    rc, text, _ = run_cli(argv + ["-o", out_file])
    assert rc == 0 and text == header_text(want, 3)
    with open(out_file) as fh:
        assert fh.read() == sample_text(cohort, coords)
    # the defaults are -p 10 --extra 8 --seed 0; another seed and no centring are read
    rc, text, _ = run_cli(["pca", "-x", cohort["base"], "--summary-only"])
    assert rc == 0 and text == header_text(ref_pca(rows, 10, extra=8, tol=1e-9, max_iter=500), 10)
    want2 = ref_pca(rows, 2, extra=2, center=False, seed=5, tol=1e-6, max_iter=3)
    rc, text, _ = run_cli(["pca", "-x", cohort["base"], "-p", "2", "--extra", "2", "--no-center", "--seed", "5", "--tolerance", "1e-6",
                           "--max-iterations", "3", "--summary-only"])
    assert rc == 0 and text == header_text(want2, 2) and "iterations 3\tconverged no" in text
    # the searcher's own call gives the same object
    pca = searcher.pca_samples(searcher.principal_axes(3, extra=5))
    assert pca.axes.tobytes() == want["axes"].tobytes() and pca.coords.tobytes() == coords.tobytes()
    assert pca.samples == [cohort["inv"][i] for i in range(N_INDEX)] and pca.stats["iterations"] == want["iterations"]


def test_within_labels_and_the_axes_file(cohort, searcher, rows):  # noqa: F811
    from morna_amd.search import format_pca_label_means, load_pca_axes, pca_label_means
    allow = np.zeros(N_INDEX, bool)
    allow[[cohort["id_map"][s] for s in cohort["some"]]] = True
    want = ref_pca(rows, 2, extra=4, tol=1e-9, max_iter=500, allow=allow)
    coords = ref_project(want["axes"], want["mean"], rows.astype(np.float64))
    assert want["fitted"] == len(cohort["some"]) < N_INDEX
    argv = ["pca", "-x", cohort["base"], "-p", "2", "--extra", "4", "--within", cohort["some_file"]]
    rc, text, err = run_cli(argv)
    assert rc == 0 and "restriction: %d of %d samples allowed" % (len(cohort["some"]), N_INDEX) in err
    assert text == header_text(want, 2) + sample_text(cohort, coords)                 # every sample is still listed
    # --labels: the label column and the block of means
    labels = dict((s, label) for label, members in cohort["groups"] for s in members)
    item_label = np.full(N_INDEX, -1, np.int32)
    for l, (_, members) in enumerate(cohort["groups"]):
        item_label[[cohort["id_map"][s] for s in members]] = l
    means = pca_label_means([label for label, _ in cohort["groups"]], item_label, coords)
    assert [count for _, count, _ in means] == [len(members) for _, members in cohort["groups"]]
    first = coords[item_label == 0]
    assert means[0][2] == pytest.approx(first.mean(axis=0).tolist(), rel=1e-12)
    axes_file = str(cohort["dir"] / "axes.npz")
    rc, text, _ = run_cli(argv + ["--labels", cohort["groups_file"], "--save-axes", axes_file])
    assert rc == 0 and text == header_text(want, 2) + sample_text(cohort, coords, labels) + format_pca_label_means(means)
    rc, text, _ = run_cli(argv + ["--labels", cohort["groups_file"], "--summary-only"])
    assert rc == 0 and text == header_text(want, 2) + format_pca_label_means(means)
    # --axes: nothing is fitted, the same lines
    saved = load_pca_axes(axes_file, rows.shape[1])
    assert saved.axes.tobytes() == want["axes"].tobytes() and saved.mean.tobytes() == want["mean"].tobytes()
    rc, text, err = run_cli(["pca", "-x", cohort["base"], "--axes", axes_file])
    assert rc == 0 and "restriction" not in err
    assert text == header_text(want, 2) + sample_text(cohort, coords)
    with pytest.raises(ValueError, match="no file of --save-axes|dimension"):
        bad = str(cohort["dir"] / "bad.npz")
        np.savez(bad, axes=want["axes"])
        run_cli(["pca", "-x", cohort["base"], "--axes", bad])


def test_queries_and_the_other_commands(cohort, searcher, rows):  # noqa: F811
    ids = cohort["ids"]
    rc, search_before, _ = run_cli(["search", "-x", cohort["base"], "-q", str(ids[5]), "-d", "-e", "-r", "5"])
    rc2, cluster_before, _ = run_cli(["cluster", "-x", cohort["base"], "-k", "3", "--seed", "1", "--summary-only"])
    assert rc == 0 and rc2 == 0
    want = ref_pca(rows, 2, extra=4, tol=1e-9, max_iter=500)
    argv = ["pca", "-x", cohort["base"], "-p", "2", "--extra", "4", "--summary-only"]
    # --intropolis: a line per sample of the file, the coordinates of the rows queries_from_intropolis stages
    batch = searcher.queries_from_intropolis(cohort["queries_file"])
    r64, _ = searcher.annoy_index.get_query_rows()
    placed = searcher.annoy_index.pca_project(want["axes"], want["mean"])
    assert placed.tobytes() == ref_project(want["axes"], want["mean"], r64).tobytes() and len(batch.ext_ids) == len(placed) > 0
    rc, text, _ = run_cli(argv + ["--intropolis", cohort["queries_file"]])
    assert rc == 0
    assert text == header_text(want, 2) + "".join("# query %s\t%s\n" % (q, "\t".join(str(c) for c in row))
                                                  for q, row in zip(batch.ext_ids, placed.tolist()))
    # a stream: the junctions of one indexed sample as -f raw, featurised as `search` does
    import io
    from morna_amd import cli
    juncs, covrs = cohort["tables"]
    sample = ids[7]
    raw = "".join("%s\t%s\t%s\t%s\n" % (tuple(cohort["lines"][j].split("\t")[:3]) + (c,)) for j, c in zip(juncs[sample], covrs[sample]))
    raw += "chrUn\t1\t2\t8\n"
    assert len(juncs[sample]) > 5
    cli._hash_stream(searcher, cli._stream_parser("raw")(io.StringIO(raw)))
    vector = np.array([searcher.query_sample], dtype=np.float64)
    assert vector.any()
    own = ref_project(want["axes"], want["mean"], vector)[0]
    rc, text, _ = run_cli(argv + ["-f", "raw"], stdin_text=raw)
    assert rc == 0 and text == header_text(want, 2) + "# query stdin\t%s\n" % "\t".join(str(c) for c in own.tolist())
    rc, search_after, _ = run_cli(["search", "-x", cohort["base"], "-q", str(ids[5]), "-d", "-e", "-r", "5"])
    rc2, cluster_after, _ = run_cli(["cluster", "-x", cohort["base"], "-k", "3", "--seed", "1", "--summary-only"])
    assert rc == 0 and rc2 == 0 and search_after == search_before and cluster_after == cluster_before
