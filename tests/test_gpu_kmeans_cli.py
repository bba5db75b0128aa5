"""`morna cluster` on the command line, on the 600-sample cohort of test_gpu_restrict_cli.py: the whole text
against the text built from MornaSearch.cluster_samples (whose arrays test_gpu_kmeans.py compares with the contract), the -o
file as a partition that the other commands read, --init-ids, --within, and `search` left as it was.  -m gpu"""
import numpy as np
import pytest

from kmeans_ref import ref_kmeans
from test_gpu_junctions import run_cli
from test_gpu_restrict_cli import N_INDEX, cohort  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def searcher(cohort):  # noqa: F811
    from morna_amd.search import MornaSearch
    return MornaSearch(cohort["base"])


def expected_text(c, summary_only=False):
    out = ["# clusters %d\titerations %d\tconverged %s\tsamples %d\tmean distance %s\n"
           % (len(c.groups), c.iterations, "yes" if c.converged else "no", c.n_samples, c.mean)]
    for (label, _), size, mean, centre in zip(c.groups, c.sizes, c.means, c.centres):
        out.append("%s\t%d\t%s\t%s\n" % (label, size, "-" if mean is None else mean, "-" if centre is None else centre))
    if not summary_only:
        for sample_id, j, d in c.samples:
            out.append("%s\t%s\t%s\n" % (sample_id, c.groups[j][0], d))
    return "".join(out)


def test_whole_text_and_the_groups_file(cohort, searcher):  # noqa: F811
    from morna_amd.junctions import parse_groups_file
    from morna_amd.search import cluster_seed_items
    c = searcher.cluster_samples(4, seed=1)
    # the arrays behind the text are the contract's
    X = searcher.annoy_index.get_items()
    seeds = cluster_seed_items(range(N_INDEX), 4, 1)
    want = ref_kmeans(X, seeds, 100)
    inv = cohort["inv"]
    assert [[cohort["id_map"][s] for s in members] for _, members in c.groups] == \
        [np.nonzero(want["assign"] == j)[0].tolist() for j in range(4)]
    assert [d for _, _, d in c.samples] == want["dist"].tolist() and [j for _, j, _ in c.samples] == want["assign"].tolist()
    assert (c.iterations, c.converged, c.sizes) == (want["iterations"], want["converged"], want["sizes"].tolist())
    assert [label for label, _ in c.groups] == ["c0000", "c0001", "c0002", "c0003"] and c.n_samples == N_INDEX
    for j in range(4):
        members = np.nonzero(want["assign"] == j)[0]
        total = 0.0
        for i in members:
            total += float(want["dist"][i])
        assert c.means[j] == total / len(members)
        assert c.centres[j] == inv[int(members[np.argmin(want["dist"][members])])]
    out_file = str(cohort["dir"] / "clusters.tsv")
    rc, text, _ = run_cli(["cluster", "-x", cohort["base"], "-k", "4", "--seed", "1", "-o", out_file])
    assert rc == 0 and text == expected_text(c)
    rc, text, _ = run_cli(["cluster", "-x", cohort["base"], "-k", "4", "--seed", "1", "--summary-only"])
    assert rc == 0 and text == expected_text(c, summary_only=True)
    groups = parse_groups_file(out_file)
    assert groups == c.groups
    assert sorted(s for _, members in groups for s in members) == cohort["ids"]
    # `labels` reads it: every cluster's size is its query count
    rc, text, _ = run_cli(["labels", "-x", cohort["base"], "--labels", out_file, "--all", "--summary-only"])
    assert rc == 0
    rows = dict((line.split("\t")[0], int(line.split("\t")[1])) for line in text.splitlines() if line.startswith("c0"))
    assert rows == dict((label, len(members)) for label, members in groups)


def test_init_ids_within_and_search_unchanged(cohort, searcher):  # noqa: F811
    ids = cohort["ids"]
    rc, before, _ = run_cli(["search", "-x", cohort["base"], "-q", str(ids[5]), "-d", "-e", "-r", "5"])
    assert rc == 0
    init = [ids[7], ids[300], ids[512]]
    init_file = str(cohort["dir"] / "init.txt")
    with open(init_file, "w") as fh:
        fh.write("".join("%d\n" % s for s in init))
    c = searcher.cluster_samples(init_ids=init)
    X = searcher.annoy_index.get_items()
    want = ref_kmeans(X, [cohort["id_map"][s] for s in init], 100)
    assert [j for _, j, _ in c.samples] == want["assign"].tolist() and c.iterations == want["iterations"]
    rc, text, _ = run_cli(["cluster", "-x", cohort["base"], "--init-ids", init_file])
    assert rc == 0 and text == expected_text(c)
    # --within: only the listed samples are partitioned
    r = searcher.restriction(within=cohort["some"])
    c = searcher.cluster_samples(3, seed=2, restriction=r)
    assert c.n_samples == len(cohort["some"]) and sorted(s for _, members in c.groups for s in members) == sorted(cohort["some"])
    rc, text, err = run_cli(["cluster", "-x", cohort["base"], "-k", "3", "--seed", "2", "--within", cohort["some_file"],
                             "--max-iterations", "50"])
    assert rc == 0 and "restriction: %d of %d samples allowed" % (len(cohort["some"]), N_INDEX) in err
    c50 = searcher.cluster_samples(3, seed=2, restriction=r, max_iterations=50)
    assert text == expected_text(c50)
    rc, after, _ = run_cli(["search", "-x", cohort["base"], "-q", str(ids[5]), "-d", "-e", "-r", "5"])
    assert rc == 0 and after == before
