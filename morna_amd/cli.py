"""`morna index` / `morna search` / `morna junctions` / `morna recovery` / `morna supersample` / `morna recall` / `morna hashing` / `morna labels` / `morna mixture` / `morna explain` / `morna pca` command line on the MI355X library.

Mirrors the reference's parser and dispatch (commanderson/morna
morna.py:867-1054, 1338-1638): same subcommands, flag names, defaults and output
format, including the metadata join (-m) and the convergence back-off loop
(-c / -ch, sam input only, `search` only).

`junctions` searches as `search` does and then pools the junctions of the results
(morna.py:1486-1638): those found in at least a share of the result samples, or
covered often enough in one of them, written as an intropolis-like splice file
for the aligner's second pass.  The junctions-by-sample databases it reads are
one file here, <basename>.junc.mor, written by `index --junction-store` (-b, the
buffer size of the reference's sqlite writer, is accepted and ignored), and the
filter runs on the GPU for all queries of a batch at once.  Differences from the
reference, all deliberate: its debug prints (shard ids, list lengths) are not
reproduced, an empty retained set writes an empty splice file (the reference
dies in ordered_junctions.pop(0)), -i is optional, and -c is refused.

`recovery` answers the question `junctions` leaves open -- which --junction-filter and -r to use on an index: it
searches as `search` does, and prints for every pair of a grid of filters how many junctions the results give back and
how many of the query's true junctions are among them (the columns junction_recovery_performance.py of the
reference's tests/ prints for one run of its aligner pipeline).  The truth is the query sample's own row of the
store, the sample itself left out of its results (-q / --query-ids), or the same sample in a second, deeper
intropolis file (--intropolis shallow --truth deep).  One pass on the GPU per run, whatever the size of the grid.
--results-sweep 5,10,20 tabulates those result counts too from the same pass: the lists are the prefixes of the one search
-r deep (for -e the lists of separate -r runs; for the approximate search, whose default search_k grows with -r, the
prefixes of the deeper and so better search).

`supersample` is create_supersample.py of the reference's tests/ on the junction store: for a list of sample ids
(--sample-ids, that script's file) or several labelled lists (--groups), the coverage of every junction summed over the
listed samples, written as that script writes it -- "chrom start end sum" for every line of --junction-file, the same
bytes -- from one pass on the GPU over the listed samples' rows and one pass over the file.  `search --supersamples
groups.tsv` searches with those sums directly, one block per group, without the files in between.  Differences from that
script, deliberate: its progress prints are not reproduced, and a sample id the store lacks is an error naming it (the
script sums nothing for it, silently).

`search --downsample 0.5,0.1` and `recovery --downsample 0.5,0.1` (with -q or --query-ids) ask their question at the depth it
is about: each query is the sample's row of the junction store with every read of every junction kept independently with
that probability -- binomial thinning of the coverages, made on the GPU by a counter-based integer hash, so the same
--downsample-seed keeps the same reads, and a lower rate keeps a subsample of a higher one's.  It stands in for
downsample_fastqs.py of the reference's tests/ and the aligner run after it, which keep a fixed number of reads of the fastq;
here the number kept is binomial and reads that span no junction do not exist.  `recovery --downsample` is that script's
downsample -> align -> recover experiment in one call: the truth is the sample's full row, or with --lost-only the junctions
of it the thinned row no longer holds.

`--within ids.txt` / `--without ids.txt` (`search`, `junctions`, `recovery`; every query kind, -e, the approximate search and
--unhashed) answer only with, or never with, the listed samples; `--leave-out-groups groups.tsv` (with -q, --query-ids and
--downsample) never answers a query with a sample of its own group -- a donor's other tissues, a study's replicates -- the
query included, and `recovery` then asks for exactly -r results instead of -r + 1 with the query dropped.  The searches
themselves are restricted on the GPU; the output format is unchanged, one line on stderr says what the
restriction holds.  Without --search-k an allow-list searches with n_trees * r * ceil(n / n_allowed) instead of 100.

`recall` answers what --n-trees and --search-k buy on an index: for every pair of --trees x --search-ks it prints how many of
the exact search's -r results the approximate search over the first t trees with that search_k returns, with the candidates
and hyperplane dots it spent, per query and over all queries -- the comparison experiment 3 of the reference's tests/README.md
makes by eye from five indexes and fifty result files.  One index, one exact search and one sweep on the GPU (DESIGN.md 8,
N11): tree i of a forest does not depend on the trees behind it, so the first t trees of the index ARE the index --n-trees t
builds.  `search --use-trees t` searches with those trees alone.

`hashing` answers what --features costs on an index: for every width of its --features list it hashes the index's items again
at that width, on the GPU and straight from the junction store (the weights of <basename>.jw.mor, the line hashes of
--junction-file), and prints how many of a sample's unhashed neighbours (`search --unhashed`) the exact search in that hashed
space returns, the mean distance error over the shared ones, with --n-trees the same for a forest search, and over all items
the mean and variance of hashed norm / unhashed norm -- experiment 2 of the reference's tests/README.md (test_norm_estimator.py)
on real rows.  One index; the population is the index's items at every width.

`labels` answers whether a sample's expression pattern resembles the samples of its tissue or cell type -- the second purpose
the reference's README gives `search`, for uncovering contamination and mislabelling: with a sample -> label table (--labels,
a groups file) it prints for every query the labels nearest to it by mean angular distance to their samples and, for a query
that is a sample of the index, its silhouette -- (b - a) / max(a, b), a the mean distance to the other samples of its own
label, b to those of the nearest other one -- and whether the nearest label is its own; over all queries a row per label,
and with --matrix the map of mean distances between labels.  One scan of the index on the GPU that keeps, per query and
label, an integer sum of all distances instead of the k smallest.

`mixture` answers the contamination half of that purpose: it writes every query as a non-negative blend of the centroids of
the labels (a non-negative least squares fit on the unit sphere, fp64, on the GPU) and prints the weights,
their shares, how far the blend stays from the query, and whether a second label holds a share of at least --min-share.  A
query that is a sample of the index is left out of its own label's centroid.

`explain` answers the question left after every search -- why is this sample near mine: it searches as `search` does with the
same flags (or takes the samples of --against, the follow-up to a line of `morna pairs`) and prints for every (query, result)
pair the unhashed distance beside the search's own, the number of junctions both hold, the share of either sample's squared
TF-IDF weight that lies outside those, and under it the --top junctions that carry most of the cosine, each with both
coverages, its weight and its share.  Every pair of every query in one call on the GPU, from the junction store and its
weights; the reference has no counterpart.

`pca` gives a cohort its picture: the p leading principal axes of the unit-scaled index rows, fitted on the GPU by a
deterministic block power iteration, the share of the variance along each, and every indexed sample's
coordinates on them -- with --labels the label beside them and the labels' mean coordinates.  --within / --without choose
the samples the axes are fitted to; every sample is still placed.  --save-axes keeps the axes, --axes reads them back and
places the samples of --intropolis, or a stream, on the axes of the cohort.  It has a parser of its own (build_pca_parser):
main() hands it everything behind the word "pca".

One deliberate difference in the back-off loop: when the stream ends without
convergence the reference's quiet branch prints the results of the LAST CHECKPOINT
(morna.py:1452, a NameError if no checkpoint was reached) while its verbose branch
finalises the whole query and searches again (morna.py:1421-1427); both branches
here do the latter.

    python -m morna_amd.cli index --intropolis junctions.tsv.gz -x idx -s 9662 --n-trees 10
    python -m morna_amd.cli search -x idx -q 1234 -d
    python -m morna_amd.cli search -x idx --intropolis new_samples.tsv.gz -e -d
    cat query.bed | python -m morna_amd.cli search -x idx -f bed --exact -d
    python -m morna_amd.cli index --intropolis junctions.tsv.gz -x idx -s 9662 --junction-store
    python -m morna_amd.cli junctions -x idx -p1 pass1.sam --junction-file junctions.tsv.gz -sf splices.txt
    python -m morna_amd.cli junctions -x idx --intropolis new_samples.tsv.gz --junction-file junctions.tsv.gz -sf splices
    python -m morna_amd.cli recovery -x idx --query-ids 12,34,56 -r 20 --grid 0,.05,.5:1,5,50
    python -m morna_amd.cli recovery -x idx --query-ids 12,34,56 -r 64 --results-sweep 5,10,20,40,64 --summary-only
    python -m morna_amd.cli recovery -x idx --intropolis shallow.tsv.gz --truth deep.tsv.gz --junction-file junctions.tsv.gz
    python -m morna_amd.cli supersample -x idx --sample-ids pancreas.txt --junction-file junctions.tsv.gz -o pancreas.qry
    python -m morna_amd.cli search -x idx --supersamples tissues.tsv --junction-file junctions.tsv.gz -e -d
    python -m morna_amd.cli search -x idx --query-ids 12,34 --downsample 0.5,0.1,0.01 --junction-file junctions.tsv.gz -d
    python -m morna_amd.cli recovery -x idx --query-ids 12,34 -r 20 --downsample 0.5,0.1,0.01 --junction-file junctions.tsv.gz --lost-only
    python -m morna_amd.cli search -x idx --intropolis new_samples.tsv.gz --within gtex_ids.txt -e -d
    python -m morna_amd.cli recovery -x idx --query-ids 12,34 -r 20 --leave-out-groups donors.tsv
    python -m morna_amd.cli search -x idx -q 1234 --use-trees 50 --search-k 1000 -d
    python -m morna_amd.cli recall -x idx --sample 100 -r 20 --trees 10,20,50,100,all --search-ks 100,200,500,1000,4000 --summary-only
    python -m morna_amd.cli hashing -x idx --junction-file junctions.tsv.gz --sample 100 -r 20 --features 500,1000,3000,8192,index
    python -m morna_amd.cli labels -x idx --labels tissues.tsv --all --matrix --summary-only
    python -m morna_amd.cli labels -x idx --labels tissues.tsv --intropolis new_samples.tsv.gz --top 3
    python -m morna_amd.cli mixture -x idx --labels tissues.tsv --all --matrix --summary-only
    python -m morna_amd.cli mixture -x idx --labels tissues.tsv --query-ids 17,42 --top 3 --min-share 0.1
    python -m morna_amd.cli search -x idx -e --max-distance 0.15 --query-ids 17,42 -d
    python -m morna_amd.cli pairs -x idx --max-distance 0.05 --leave-out-groups donors.tsv --clusters
    python -m morna_amd.cli explain -x idx --junction-file junctions.tsv.gz --query-ids 17,42 -r 20 --top 10
    python -m morna_amd.cli explain -x idx --junction-file junctions.tsv.gz -q 17 --against 42,1234 --summary-only
    python -m morna_amd.cli pca -x idx -p 10 --labels tissues.tsv --save-axes cohort.npz -o coords.tsv
    python -m morna_amd.cli pca -x idx --axes cohort.npz --intropolis new_samples.tsv.gz --summary-only
"""
import argparse
import sys

_help_intro = """morna searches for known RNA-seq samples with exon-exon junction expression
patterns similar to those in a query sample (MI355X build of the index/search hot path).
"""


class _StoreGiven(argparse.Action):
    """store, and note in <dest>_given that the flag was on the command line"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


# ---- the parser -------------------------------------------------------------------------------------------------------------
_CONST = dict(action='store_const', const=True, default=False)
_FILE = dict(metavar='<file>', type=str, required=False, default=None)
_INT = dict(metavar='<int>', type=int, required=False, default=None)
# the flags several commands take, by dest: their names and everything but the help text, which is every command's own
_SHARED = {
    'basename': (('-x', '--basename'), dict(metavar='<idx>', type=str, required=True)),
    'verbose': (('-v', '--verbose'), _CONST),
    'query_id': (('-q', '--query-id'), _INT),
    'query_ids': (('--query-ids',), dict(metavar='<ids>', type=str, required=False, default=None)),
    'sample': (('--sample',), _INT),
    'sample_seed': (('--sample-seed',), dict(metavar='<int>', type=int, required=False, default=0, action=_StoreGiven)),
    'all_items': (('--all',), dict(dest='all_items', **_CONST)),
    'intropolis': (('--intropolis',), _FILE),
    'format': (('-f', '--format'), dict(metavar='<choice>', type=str, required=False, default='sam')),
    'exact': (('-e', '--exact'), _CONST),
    'unhashed': (('--unhashed',), _CONST),
    'search_k': (('--search-k',), dict(metavar='<int>', type=int, required=False, default=100, action=_StoreGiven)),
    'supersamples': (('--supersamples',), _FILE),
    'within': (('--within',), _FILE),
    'without': (('--without',), _FILE),
    'leave_out_groups': (('--leave-out-groups',), _FILE),
    'metadata': (('-m', '--metadata'), _CONST),
    'summary_only': (('--summary-only',), _CONST),
    'device': (('--device',), dict(type=str, default='0')),
}
# what the commands after `search` say of their query sources
_SOURCE_HELP = dict(query_id='the query is the sample already in the index with this sample id',
                    query_ids='comma-separated sample ids already in the index',
                    sample='this many distinct indexed samples, drawn with numpy.random.RandomState(--sample-seed)',
                    sample_seed='the seed of --sample (default 0)',
                    all_items='every sample of the index is a query',
                    intropolis='every sample of this (gzipped) intropolis file is a query',
                    format='one of {sam, bed, raw}: the format of a query read from stdin, when no other query is named')
_DEVICE_HELP = 'HIP device ordinal'
_SUMMARY_HELP = 'print only the table over all queries'
_COMPARED_HELP = 'the number of nearest neighbor results compared (at most 256)'
_UNSHARDED_HELP = 'path to junction index basename (an index without row shards)'
_STORE_INDEX_HELP = 'basename of an index built with --junction-store (an index without row shards)'


def _add_flags(subparser, **helps):
    """The shared flags named, by dest and in this order, each with the help text this command gives it."""
    for dest, text in helps.items():
        names, rest = _SHARED[dest]
        subparser.add_argument(*names, help=text, **rest)


def _add_sources(subparser, *dests):
    """The query-source flags named, with the help text of the commands after `search`."""
    _add_flags(subparser, **dict((dest, _SOURCE_HELP[dest]) for dest in dests))


def _add_refused(subparser, *dests):
    """Flags of `search` that have no meaning for this command: taken, and hidden, so that they can be refused with a reason."""
    for dest in dests:
        names, rest = _SHARED[dest]
        if rest is _CONST:
            subparser.add_argument(*names, help=argparse.SUPPRESS, **_CONST)
        else:
            subparser.add_argument(*names, type=str, required=False, default=None, help=argparse.SUPPRESS)


def _add_junction_file(subparser, text='path to the (gzipped) intropolis file the index was made from', required=True, **rest):
    subparser.add_argument('--junction-file', type=str, metavar='<gz>', required=required, help=text, **rest)


def _add_results(subparser, text, given=True):
    """-r; given: note in results_given that it was on the command line."""
    subparser.add_argument('-r', '--results', metavar='<int>', type=int, required=False, default=20, help=text,
                           **(dict(action=_StoreGiven) if given else {}))


def add_search_parameters(subparser):
    _add_flags(subparser, basename='path to junction index basename for search', verbose='be talkative',
               search_k='a larger value makes for more accurate search', format='one of {sam, bed, raw}')
    subparser.add_argument('-d', '--distances', action='store_const', const=True, default=False,
                           help='include distances to nearest neighbors')
    _add_flags(subparser, metadata='display results mapped to metadata')
    subparser.add_argument('-c', '--convergence-backoff', metavar='<int>', type=int, required=False, default=None,
                           help='attempt to converge on a solution with this backoff interval '
                                '(check after c, then 2c, then 4c, and stop when no change)')
    subparser.add_argument('-ch', '--checkpoint', metavar='<int>', type=int, required=False, default=0,
                           help='do not start backoff until this point (check at checkpoint, '
                                'then checkpoint + c, then continue exponential backoff)')
    _add_flags(subparser, query_id='search for nearest neighbors to the sample already in the index with this sample id',
               exact='exact nearest neighbor search within the morna index')
    _add_results(subparser, 'the number of nearest neighbor results to return')
    subparser.add_argument('-rl', '--rawlist', action='store_const', const=True, default=False,
                           help='regurgitate junction list for input sample instead of performing search')
    _add_flags(subparser,
               intropolis='search every sample of this (gzipped) intropolis file at once: one block per sample, '
                          '"# query <sample id>" and then what -f raw prints for that sample\'s junctions '
                          '(-f is ignored)',
               query_ids='comma-separated sample ids already in the index, searched together: one block per id, '
                         '"# query <id>" and then what -q <id> prints',
               supersamples='search with pooled samples: a groups file, "<label><TAB><id>,<id>,..." per line; every '
                            'group\'s samples are summed junction by junction on the GPU (needs the store of `index '
                            '--junction-store`) and the sums searched together: one block per group, "# query <label>" '
                            'and then what --intropolis prints for a sample with those sums (`search` only; needs '
                            '--junction-file)',
               unhashed='rank by the TF-IDF cosine distance over the junctions themselves, one dimension per '
                        'line of the indexed file, instead of the hashed features (needs the store and weights '
                        'of `index --junction-store`; `search` only)')
    subparser.add_argument('--downsample', metavar='<p1,p2,...>', type=str, required=False, default=None,
                           help='with -q or --query-ids: search with each sample\'s row of the junction store at these '
                                'fractions of its depth (1 to 16 rates in [0, 1]): every read of every junction is kept '
                                'independently with that probability, on the GPU and reproducibly (needs the store of `index '
                                '--junction-store`, and --junction-file unless --unhashed); one block per id and rate, '
                                '"# query <id><TAB>keep <rate>" and then what --intropolis prints for a sample with the '
                                'thinned coverages (`search` and `recovery`)')
    subparser.add_argument('--downsample-seed', metavar='<int>', type=int, required=False, default=8675309, action=_StoreGiven,
                           help='the seed of --downsample (default 8675309); the same seed gives the same reads')
    _add_flags(subparser,
               within='answer only with the samples this file lists, one integer sample id per line',
               without='never answer with a sample this file lists, one integer sample id per line',
               leave_out_groups='with -q, --query-ids and --downsample: a groups file, "<label><TAB><id>,<id>,..." per line; '
                                'a query is never answered with a sample of its own group, itself included, and a query '
                                'sample the file does not name is a group of its own.  `recovery` then asks for exactly -r '
                                'results instead of -r + 1 with the query dropped',
               device='HIP device ordinal; for an index built with --shards also a list, "0,1,2,3": the shards are '
                      'dealt to these devices in turn')


def build_parser():
    parser = argparse.ArgumentParser(description=_help_intro)
    subparsers = parser.add_subparsers(dest='subparser_name',
                                       help='subcommands; add "-h" or "--help" after a subcommand for its parameters')
    index_parser = subparsers.add_parser('index', help='creates a morna index')
    search_parser = subparsers.add_parser('search', help='searches a morna index')
    index_parser.add_argument('--intropolis', metavar='<file>', type=str, required=True,
                              help='path to gzipped file recording junctions across samples in intropolis format')
    index_parser.add_argument('-x', '--basename', metavar='<str>', type=str, required=False, default='morna',
                              help='basename path of junction index files to create')
    index_parser.add_argument('--features', metavar='<int>', type=int, required=False, default=3000,
                              help='dimension of feature space')
    index_parser.add_argument('--n-trees', metavar='<int>', type=int, required=False, default=200,
                              help='number of annoy trees')
    index_parser.add_argument('-s', '--sample-count', metavar='<int>', type=int, required=False, default=None,
                              help='optionally specify number of unique samples to speed indexing')
    index_parser.add_argument('-t', '--sample-threshold', metavar='<int>', type=int, required=False, default=100,
                              help='minimum number of samples in which a junction should appear')
    index_parser.add_argument('-b', '--buffer-size', metavar='<int>', type=int, required=False, default=1024,
                              help='accepted for compatibility and ignored: the junctions-by-sample store is written '
                                   'in one piece (--junction-store)')
    _add_flags(index_parser, verbose='be talkative')
    index_parser.add_argument('-m', '--metafile', metavar='<file>', type=str, required=False, default=None,
                              help='path to metadata file with sample index in first column '
                                   'and other keywords in other columns, whitespace delimited')
    index_parser.add_argument('--device', type=int, default=0, help='HIP device ordinal')
    index_parser.add_argument('--python-parse', action='store_const', const=True, default=False,
                              help='tokenise the intropolis file with the Python loop of the reference '
                                   'instead of the native pre-pass (same index either way)')
    index_parser.add_argument('--cache', metavar='<file>', type=str, required=False, default=None,
                              help='binary pre-tokenised cache of the intropolis file: reused when it matches the '
                                   'file, sample count and threshold, (re)written otherwise')
    index_parser.add_argument('--shards', metavar='<int>', type=int, required=False, default=1,
                              help='cut the samples into this many contiguous row shards, each with its own matrix + '
                                   'forest file (one per GPU); global idf and internal ids, so the shards together are '
                                   'the index.  Under torchrun with WORLD_SIZE equal to --shards every rank builds its '
                                   'own shard on its own GPU; otherwise one process builds them one after the other')
    index_parser.add_argument('--junction-store', action='store_const', const=True, default=False,
                              help='also write <basename>.junc.mor, the junctions-by-sample store `morna junctions` reads '
                                   '(a second parse of the file, every line kept, transposed on the GPU); without this '
                                   'flag a store left by an earlier index of the same basename is removed')
    add_search_parameters(search_parser)
    _add_junction_file(search_parser, 'with --unhashed and a query that is not already in the index (a stream, --intropolis), '
                       'with --supersamples, and with --downsample unless --unhashed: path to the (gzipped) intropolis file the index was made '
                       'from, which names the junction of every line', required=False, default=None, dest='unhashed_junction_file')
    search_parser.add_argument('--use-trees', metavar='<int>', type=int, required=False, default=None,
                               help='search with the first <int> trees of the index only: the answer of an index built with '
                                    '--n-trees <int> from the same file (approximate search on an index without row shards; '
                                    'not with -e, --unhashed, --within, --without or --leave-out-groups)')
    search_parser.add_argument('--max-distance', metavar='<float>', type=str, required=False, default=None,
                               help='with -e: every sample within this exact distance of the query instead of the -r nearest, '
                                    'in the format of the -e output (an explicit -r caps the list); for -q and --query-ids the '
                                    'exact search by sample (not with --unhashed, --use-trees, -c or an index of row shards)')
    junctions_parser = subparsers.add_parser('junctions', help='searches a morna index and pools the junctions of the '
                                                               'results for a second alignment pass')
    add_search_parameters(junctions_parser)                    # morna.py:1023
    junctions_parser.set_defaults(unhashed_junction_file=None, use_trees=None, max_distance=None)   # (search's --junction-file: the unhashed search's; not this one; --use-trees is search's alone)
    junctions_parser.add_argument('-i', '--index', metavar='<idx>', type=str, required=False, default=None,
                                  help='accepted for compatibility and ignored (the aligner\'s index; morna.py:1025)')
    junctions_parser.add_argument('-p1', '--pass1-sam', metavar='<sam>', type=str, required=False, default="pass1.sam",
                                  help='first pass alignment file output by the aligner: the query, read in place of '
                                       'stdin when no other query is named')
    junctions_parser.add_argument('--junction-filter', type=str, required=False, default=".05,5",
                                  help='two parts separated by a comma: retain the junctions found in at least {first part} '
                                       'proportion of the result samples, or with at least {second part} coverage in any '
                                       'one result sample')
    _add_junction_file(junctions_parser)
    junctions_parser.add_argument('-sf', '--splicefile', type=str, metavar='<file>', required=True,
                                  help='intropolis-like output file with the retained junctions and, as one more field, '
                                       'the ranks of the results that hold each; a batch (--intropolis, --query-ids) '
                                       'writes <file>.<sample id> per query')
    recovery_parser = subparsers.add_parser('recovery', help='searches a morna index and tabulates, over a grid of junction '
                                                             'filters, how many of a query\'s true junctions its results '
                                                             'give back')
    add_search_parameters(recovery_parser)
    recovery_parser.set_defaults(unhashed_junction_file=None, use_trees=None, max_distance=None)
    recovery_parser.add_argument('--grid', type=str, required=False, default=None,
                                 help='the filters to tabulate, "<f1>,<f2>,...:<c1>,<c2>,...": every frequency with every '
                                      'coverage (at most 15 coverages); default 0,.05,.1,.2,.3,.5,.75,1:1,2,3,5,10,20,50,1000')
    recovery_parser.add_argument('--truth-coverage', metavar='<int>', type=int, required=False, default=1,
                                 help='a junction is true for a query when the truth covers it at least this many times')
    recovery_parser.add_argument('--truth', type=str, metavar='<gz>', required=False, default=None,
                                 help='with --intropolis: the (gzipped) intropolis file that holds the true junctions of the '
                                      'same sample ids (the samples sequenced deeply)')
    _add_junction_file(recovery_parser, 'with --truth and with --downsample: path to the (gzipped) intropolis file the index was made from, which '
                       'names the junction of every line', required=False, default=None)
    _add_flags(recovery_parser, summary_only=_SUMMARY_HELP)
    recovery_parser.add_argument('--results-sweep', type=str, metavar='<p1,p2,...>', required=False, default=None,
                                 help='tabulate these result counts (at most 8, each at most -r) from the one search -r deep '
                                      'and one pass over its results: a block per count for every query, then a table over '
                                      'all queries per count')
    recovery_parser.add_argument('--lost-only', action='store_const', const=True, default=False,
                                 help='with --downsample: the truth of a query is only the junctions of its full row (at '
                                      '--truth-coverage) that its thinned row does not hold, those the shallow run lost. '
                                      'Precision is then against the lost junctions only, so a result that gives back a '
                                      'junction the query kept counts as a false positive: recall is the number of interest')
    recall_parser = subparsers.add_parser('recall', help='tabulates the recall of the approximate search against the exact one '
                                                         'over a grid of tree counts and search_k values, from one index')
    _add_flags(recall_parser, basename=_UNSHARDED_HELP)
    _add_sources(recall_parser, 'query_id', 'query_ids', 'intropolis', 'sample', 'sample_seed')
    _add_results(recall_parser, _COMPARED_HELP, given=False)
    recall_parser.add_argument('--trees', metavar='<t1,t2,...>', type=str, required=True,
                               help='tree counts, ascending, at most 64; "all" stands for the index\'s tree count')
    recall_parser.add_argument('--search-ks', metavar='<s1,s2,...>', type=str, required=True,
                               help='search_k values, ascending, at most 64')
    _add_flags(recall_parser, summary_only=_SUMMARY_HELP, device=_DEVICE_HELP)
    hashing_parser = subparsers.add_parser('hashing', help='tabulates what each --features value costs in neighbours and in norm '
                                                           'distortion against the unhashed search, from one index with a '
                                                           'junction store')
    _add_flags(hashing_parser, basename=_STORE_INDEX_HELP)
    _add_junction_file(hashing_parser)
    _add_sources(hashing_parser, 'query_id', 'query_ids', 'sample', 'sample_seed')
    _add_results(hashing_parser, _COMPARED_HELP, given=False)
    hashing_parser.add_argument('--features', metavar='<d1,d2,...>', type=str, required=True,
                                help='hashed widths, ascending, at most 16, each 1 to 32768; "index" stands for the index\'s own')
    hashing_parser.add_argument('--n-trees', metavar='<int>', type=int, required=False, default=None,
                                help='also build a forest of this many trees at every width and search it')
    _add_flags(hashing_parser, search_k='search_k of the forest search (with --n-trees; default 100)', summary_only=_SUMMARY_HELP,
               device=_DEVICE_HELP)
    _add_refused(hashing_parser, 'exact', 'unhashed', 'within', 'without', 'leave_out_groups', 'intropolis')
    labels_parser = subparsers.add_parser('labels', help='tabulates, for every query, its mean distance to the samples of every '
                                                         'label of a sample -> label table, and how well the labels hold '
                                                         'together in the hashed space, from one scan of the index')
    _add_flags(labels_parser, basename=_UNSHARDED_HELP)
    labels_parser.add_argument('--labels', metavar='<file>', type=str, required=True,
                               help='a groups file, "<label><TAB><id>,<id>,..." per line: the samples of every label (a tissue, '
                                    'a cell type), at most 4096 labels; a sample it does not name has none')
    _add_sources(labels_parser, 'query_id', 'query_ids', 'sample', 'sample_seed', 'all_items', 'intropolis', 'format')
    labels_parser.add_argument('--top', metavar='<int>', type=int, required=False, default=3,
                               help='the nearest labels printed per query (default 3)')
    labels_parser.add_argument('--matrix', action='store_const', const=True, default=False,
                               help='append the label map: for every pair of labels (A, B) the mean distance from the queries '
                                    'of label A to the samples of label B (queries that are samples of the index only)')
    _add_flags(labels_parser, summary_only=_SUMMARY_HELP,
               within='count only the samples this file lists, one integer sample id per line',
               without='never count a sample this file lists, one integer sample id per line',
               leave_out_groups='a groups file: a query never counts a sample of its own group -- its donor, its study -- '
                                '(queries that are samples of the index only)',
               device=_DEVICE_HELP)
    mixture_parser = subparsers.add_parser('mixture', help='writes every query as a non-negative blend of the centroids of the '
                                                           'labels of a sample -> label table and says which queries are '
                                                           'mixed: a contaminated sample shows a second label with a share')
    _add_flags(mixture_parser, basename=_UNSHARDED_HELP)
    mixture_parser.add_argument('--labels', metavar='<file>', type=str, required=True,
                                help='a groups file, "<label><TAB><id>,<id>,..." per line: the samples of every label (a tissue, '
                                     'a cell type), at most 128 labels; a sample it does not name has none')
    _add_sources(mixture_parser, 'query_id', 'query_ids', 'sample', 'sample_seed', 'all_items', 'intropolis', 'format')
    mixture_parser.add_argument('--top', metavar='<int>', type=int, required=False, default=3,
                                help='the labels of the largest weights printed per query (default 3)')
    mixture_parser.add_argument('--min-share', metavar='<float>', type=float, required=False, default=0.1,
                                help='a query is mixed when its second label holds at least this share of the weights (default 0.1)')
    mixture_parser.add_argument('--tolerance', metavar='<float>', type=float, required=False, default=1e-9,
                                help='the fit stops after a sweep whose largest step is at most this (default 1e-9)')
    mixture_parser.add_argument('--max-sweeps', metavar='<int>', type=int, required=False, default=10000,
                                help='the sweeps a fit may take (default 10000)')
    mixture_parser.add_argument('--matrix', action='store_const', const=True, default=False,
                                help='append the table of mean shares: the row is the queries\' own label, the column the fitted '
                                     'label (queries that are samples of the index only)')
    _add_flags(mixture_parser, summary_only=_SUMMARY_HELP,
               within='the centroids are made of the samples this file lists only, one integer sample id per line',
               without='no centroid holds a sample this file lists, one integer sample id per line', device=_DEVICE_HELP)
    _add_refused(mixture_parser, 'exact', 'unhashed', 'leave_out_groups', 'supersamples')
    super_parser = subparsers.add_parser('supersample', help='sums the coverage of every junction over groups of indexed '
                                                             'samples (create_supersample.py on the junction store)')
    _add_flags(super_parser, basename='basename of an index built with --junction-store')
    which = super_parser.add_mutually_exclusive_group(required=True)
    which.add_argument('--sample-ids', metavar='<file>', type=str, default=None,
                       help='one integer sample id per line (the --sampleids file of create_supersample.py): one output file')
    which.add_argument('--groups', metavar='<file>', type=str, default=None,
                       help='"<label><TAB><id>,<id>,..." per line: one output file per group, <out>.<label>')
    _add_junction_file(super_parser)
    super_parser.add_argument('-o', '--output', type=str, metavar='<file>', required=True,
                              help='output file: "chrom start end sum" for every line of --junction-file')
    _add_flags(super_parser, device=_DEVICE_HELP)
    pairs_parser = subparsers.add_parser('pairs', help='lists every pair of indexed samples within a distance of each other '
                                                       '(re-submitted runs, replicates, one library under two accessions), '
                                                       'from one exact scan of the index')
    _add_flags(pairs_parser, basename=_UNSHARDED_HELP)
    pairs_parser.add_argument('--max-distance', metavar='<float>', type=str, required=True,
                              help='report the pairs at most this exact distance apart')
    _add_flags(pairs_parser, within='pair only the samples this file lists, one integer sample id per line',
               without='never pair a sample this file lists, one integer sample id per line',
               leave_out_groups='a groups file, "<label><TAB><id>,<id>,..." per line: never pair two samples of one group '
                                '(the expected pairs -- one donor, one study -- stay silent, the unexpected ones remain)',
               metadata='append both samples\' metadata keywords to every line')
    pairs_parser.add_argument('--clusters', action='store_const', const=True, default=False,
                              help='append one line per connected component of the pairs, largest first')
    _add_flags(pairs_parser, summary_only='print only the summary line (and the clusters with --clusters)', device=_DEVICE_HELP)
    cluster_parser = subparsers.add_parser('cluster', help='partitions the indexed samples into k groups by their distance in the '
                                                           'hashed space (spherical k-means on the GPU) and writes the groups '
                                                           'file that labels, --leave-out-groups and --supersamples read')
    _add_flags(cluster_parser, basename=_UNSHARDED_HELP)
    cluster_parser.add_argument('-k', '--clusters', metavar='<int>', type=int, required=False, default=None,
                                help='the number of groups, 1 to 4096 (with --init-ids: their number)')
    cluster_parser.add_argument('--seed', metavar='<int>', type=int, required=False, default=0, action=_StoreGiven,
                                help='the first centroids are random.Random(seed).sample of the samples (default 0)')
    cluster_parser.add_argument('--init-ids', metavar='<file>', type=str, required=False, default=None,
                                help='the first centroids are the samples this file lists, one integer sample id per line')
    cluster_parser.add_argument('--max-iterations', metavar='<int>', type=int, required=False, default=100,
                                help='stop after this many assignments when the groups still change (default 100)')
    _add_flags(cluster_parser, within='partition only the samples this file lists, one integer sample id per line',
               without='leave out the samples this file lists, one integer sample id per line')
    cluster_parser.add_argument('-o', '--output', metavar='<file>', type=str, required=False, default=None,
                                help='write the groups file here: "<label><TAB><id>,<id>,..." per group')
    _add_flags(cluster_parser, summary_only='print only the header and the line of every group',
               metadata='append the metadata keywords of every group\'s centre sample', device=_DEVICE_HELP)
    _add_refused(cluster_parser, 'exact', 'unhashed', 'leave_out_groups')
    explain_parser = subparsers.add_parser('explain', help='searches a morna index and prints, for every query and result, the '
                                                           'junctions behind their distance: how many they share, how much of '
                                                           'either sample lies outside those, and the junctions that carry most')
    _add_flags(explain_parser, basename=_STORE_INDEX_HELP)
    _add_junction_file(explain_parser, 'path to the (gzipped) intropolis file the index was made from: it names the junctions')
    _add_sources(explain_parser, 'query_id', 'query_ids', 'sample', 'sample_seed', 'intropolis', 'format')
    _add_results(explain_parser, 'the number of nearest neighbor results to search for and explain (default 20)')
    _add_flags(explain_parser, exact='search exactly, as `search -e` does',
               unhashed='search in the space of the junctions themselves, as `search --unhashed` does',
               search_k='a larger value makes for more accurate search')
    explain_parser.add_argument('--against', metavar='<ids>', type=str, required=False, default=None,
                                help='comma-separated sample ids of the index: no search runs, every query is explained against '
                                     'every one of them, in this order (the follow-up to a line of `morna pairs`)')
    explain_parser.add_argument('--top', metavar='<int>', type=int, required=False, default=10,
                                help='the junctions of largest contribution printed per pair, 1 to 64 (default 10)')
    _add_flags(explain_parser, within='answer only with the samples this file lists, one integer sample id per line',
               without='never answer with a sample this file lists, one integer sample id per line',
               summary_only='print only the line of every pair, not the junctions under it',
               metadata='append the metadata keywords of every result, as `search -m` does', device=_DEVICE_HELP)
    return parser


def build_pca_parser():
    """The parser of `morna pca`, a command with a parser of its own: main() hands it everything behind the word "pca"."""
    parser = argparse.ArgumentParser(prog='morna pca',
                                     description='principal axes of the indexed samples in the hashed space, fitted on the GPU, and '
                                                 'every sample\'s coordinates on them: the picture of a cohort')
    _add_flags(parser, basename=_UNSHARDED_HELP)
    parser.add_argument('-p', '--components', metavar='<int>', type=int, required=False, default=10, action=_StoreGiven,
                        help='the number of axes, 1 to 32 (default 10)')
    parser.add_argument('--extra', metavar='<int>', type=int, required=False, default=8, action=_StoreGiven,
                        help='columns iterated beside the axes: more of them, fewer iterations; -p and --extra together at most '
                             '64 (default 8)')
    parser.add_argument('--no-center', action='store_const', const=True, default=False,
                        help='do not subtract the mean sample: axes of the second moments about the origin')
    parser.add_argument('--seed', metavar='<int>', type=int, required=False, default=0, action=_StoreGiven,
                        help='the seed of the first block of columns (default 0); the same seed gives the same bytes')
    parser.add_argument('--tolerance', metavar='<float>', type=float, required=False, default=1e-9, action=_StoreGiven,
                        help='stop when no variance changed by more than this share of the largest (default 1e-9)')
    parser.add_argument('--max-iterations', metavar='<int>', type=int, required=False, default=500, action=_StoreGiven,
                        help='the iterations the fit may take (default 500)')
    _add_flags(parser, within='fit the axes to the samples this file lists only, one integer sample id per line (every sample is '
                              'still placed)',
               without='leave the samples this file lists out of the fit, one integer sample id per line')
    parser.add_argument('--labels', metavar='<file>', type=str, required=False, default=None,
                        help='a groups file, "<label><TAB><id>,<id>,..." per line: every sample\'s line carries its label, and a '
                             'block of per-label mean coordinates follows')
    _add_sources(parser, 'intropolis')
    parser.add_argument('-f', '--format', metavar='<choice>', type=str, required=False, default=None,
                        help='one of {sam, bed, raw}: place the query read from stdin in this format, featurised as `search` does')
    parser.add_argument('--save-axes', metavar='<file>', type=str, required=False, default=None,
                        help='write mean, axes, variances and the fit\'s figures to this .npz file')
    parser.add_argument('--axes', metavar='<file>', type=str, required=False, default=None,
                        help='read the axes from this file of --save-axes and fit nothing: only place samples and queries')
    parser.add_argument('-o', '--output', metavar='<file>', type=str, required=False, default=None,
                        help='write the line of every indexed sample to this file and not to stdout')
    _add_flags(parser, summary_only='print no line per indexed sample',
               metadata='append the metadata keywords of every sample', device=_DEVICE_HELP)
    return parser


# ---- the pieces the flag checks share: argparse errors, before any index is read -----------------------------------------------
_SOURCE_FLAGS = dict(query_id="-q/--query-id", query_ids="--query-ids", sample="--sample", all_items="--all", intropolis="--intropolis")
_ONE_PROCESS_REFUSAL = ("batch search is not available with one process per shard (torchrun): "
                        "run it in one process, which loads every shard of the index")


def _refuse(parser, template, flags):
    """template % flag is the parser's error for the first of `flags`, (flag, on) or (flag, on, reason), that is on; the
    reason follows a colon."""
    for flag, on, *why in flags:
        if on:
            parser.error(template % flag + "".join(": " + reason for reason in why))


def _given(args, dest):
    """The flag of a _StoreGiven action was on the command line."""
    return getattr(args, dest + "_given", False)


def _stream_flags(args):
    """-c and -rl as _refuse takes them: what only the search of one stream does."""
    return [("-c/--convergence-backoff", args.convergence_backoff is not None), ("-rl/--rawlist", args.rawlist)]


def _parse_ids(parser, text, flag="--query-ids"):
    """The ids of --query-ids (or --against); "--query-ids takes comma-separated integer sample ids (got ...)" otherwise."""
    try:
        return [int(t) for t in text.split(',')]
    except ValueError:
        parser.error("%s takes comma-separated integer sample ids (got %r)" % (flag, text))


def _parse_distance(parser, text):
    from .search import parse_max_distance
    try:
        return parse_max_distance(text)
    except ValueError as e:
        parser.error(str(e))


def _check_sample(parser, args):
    """--sample is a positive count, --sample-seed comes only with it."""
    if args.sample is None and _given(args, "sample_seed"):
        parser.error("--sample-seed cannot be used without --sample")
    if args.sample is not None and args.sample < 1:
        parser.error("--sample takes a positive number of samples (got %d)" % args.sample)


def _check_sources(parser, args, command, dests, stream):
    """The query sources of a command after `search`: one of the flags `dests` -- exactly one, or with `stream` at most one
    and -f for the query on stdin -- in the command's wording, then --query-ids parsed and --sample checked.  Returns the
    flags given."""
    given = [_SOURCE_FLAGS[dest] for dest in dests if getattr(args, dest) is not None and getattr(args, dest) is not False]
    short = [_SOURCE_FLAGS[dest].split("/")[0] for dest in dests] + (["a stream on stdin"] if stream else [])
    listed = ", ".join(short[:-1]) + " or " + short[-1]
    if stream and len(given) > 1:
        parser.error("%s takes one query source: %s (got %s)" % (command, listed, " and ".join(given)))
    if not stream and len(given) != 1:
        parser.error("%s needs exactly one query source: %s" % (command, listed) + (" (got %s)" % " and ".join(given) if given else ""))
    if stream and args.format not in ("sam", "bed", "raw"):
        parser.error("-f takes one of sam, bed, raw (got %r)" % args.format)
    if args.query_ids is not None:
        args.query_ids = _parse_ids(parser, args.query_ids)
    _check_sample(parser, args)
    return given


def _read_file(parser, parse, path):
    """parse(path), None without a path; what it raises is the parser's error."""
    if path is None:
        return None
    try:
        return parse(path)
    except (ValueError, IOError, OSError) as e:
        parser.error(str(e))


def _read_restriction(parser, args, groups=True):
    """The files of --within / --without / --leave-out-groups (groups=False: a command that takes no groups file) read into
    args.within_ids / args.without_ids / args.leave_out, None where the flag is absent, and args.restriction = None for the
    command to fill in."""
    from .junctions import parse_groups_file, parse_sample_ids_file
    args.within_ids = args.without_ids = args.leave_out = args.restriction = None
    try:
        if args.within is not None:
            args.within_ids = parse_sample_ids_file(args.within)
        if args.without is not None:
            args.without_ids = parse_sample_ids_file(args.without)
        if groups and args.leave_out_groups is not None:
            args.leave_out = parse_groups_file(args.leave_out_groups)
    except (ValueError, IOError, OSError) as e:
        parser.error(str(e))


def _check_within_without(parser, args):
    if args.within_ids is not None and args.without_ids is not None:
        both = sorted(set(args.within_ids) & set(args.without_ids))
        if both:
            parser.error("--within and --without both name sample id %d" % both[0])


def _shards(args):
    """(the index is one of row shards, WORLD_SIZE): what every shard refusal and main's tail ask."""
    import os
    return os.path.exists(args.basename + ".shards.mor"), int(os.environ.get("WORLD_SIZE", "1"))


def _refuse_shards(parser, args, refusal):
    """A command that runs in one process on an index without row shards and says so in the parser."""
    on_shards, world = _shards(args)
    if on_shards or world > 1:
        parser.error(refusal)


def _require_store(args, weights=False, parser=None):
    """The junction store next to the index and, with `weights`, the line weights of the unhashed search: the parser's error
    with a parser, IOError without."""
    import os
    from .junctions import STORE_SUFFIX, WEIGHTS_SUFFIX

    def missing(text):
        if parser is not None:
            parser.error(text)
        raise IOError(text)
    if not os.path.exists(args.basename + STORE_SUFFIX):
        missing("%s not found: this index has no junction store; build it with `morna index --junction-store`"
                % (args.basename + STORE_SUFFIX))
    if weights and not os.path.exists(args.basename + WEIGHTS_SUFFIX):
        missing("%s not found: --unhashed needs the line weights `morna index --junction-store` writes next "
                "to the junction store. They are not written when a junction repeats in the indexed file: "
                "the unhashed search is defined for files without repeated junctions" % (args.basename + WEIGHTS_SUFFIX))


# ---- the flag checks of the commands, in the order main() runs them ---------------------------------------------------------------
def _check_max_distance_flags(parser, args):
    """search --max-distance: the exact, hashed search of an index without row shards; leaves the distance in
    args.max_distance (None without the flag)."""
    if getattr(args, "max_distance", None) is None:
        return
    from .search import RADIUS_SHARDS_REFUSAL
    args.max_distance = _parse_distance(parser, args.max_distance)
    if not args.exact:
        parser.error("--max-distance cannot be used without -e/--exact: the distance is the exact search's")
    _refuse(parser, "--max-distance cannot be used with %s",
            [("--unhashed", args.unhashed), ("--use-trees", _use_trees(args) is not None)] + _stream_flags(args))
    if args.results < 1:
        parser.error("-r takes a positive number of results (got %d)" % args.results)
    _refuse_shards(parser, args, RADIUS_SHARDS_REFUSAL)


def _check_pairs_flags(parser, args):
    """`pairs`: the distance and the restriction's files, checked against each other.  Leaves the restriction's parts
    where _check_restriction_flags leaves them."""
    args.max_distance = _parse_distance(parser, args.max_distance)
    args.query_id = args.query_ids = None
    _read_restriction(parser, args)
    _check_within_without(parser, args)


def _check_cluster_flags(parser, args):
    """`cluster`: the flags of the searches that make no sense here, k or the first centroids, the restriction's files.
    Leaves the restriction's parts where _check_restriction_flags leaves them and the first centroids in
    args.init_sample_ids."""
    from .junctions import parse_sample_ids_file
    from .search import CLUSTER_SHARDS_REFUSAL, LABELS_MAX
    _refuse(parser, "cluster cannot be used with %s",
            (("-e/--exact", args.exact, "every distance of a partition is exact already"),
             ("--unhashed", args.unhashed, "the groups are formed in the hashed space, over the index's rows"),
             ("--leave-out-groups", args.leave_out_groups is not None,
              "cluster makes groups, it takes none: --within and --without choose the samples")))
    if args.init_ids is not None and _given(args, "seed"):
        parser.error("--seed and --init-ids cannot be used together")
    if args.init_ids is None and args.clusters is None:
        parser.error("cluster needs -k, the number of groups, or --init-ids")
    if args.max_iterations < 1:
        parser.error("--max-iterations takes a positive number (got %d)" % args.max_iterations)
    args.query_id = args.query_ids = None
    args.init_sample_ids = _read_file(parser, parse_sample_ids_file, args.init_ids)
    _read_restriction(parser, args, groups=False)
    if args.init_sample_ids is not None:
        if len(set(args.init_sample_ids)) != len(args.init_sample_ids):
            parser.error("--init-ids %s names a sample twice" % args.init_ids)
        if args.clusters is not None and args.clusters != len(args.init_sample_ids):
            parser.error("-k %d, but --init-ids names %d samples" % (args.clusters, len(args.init_sample_ids)))
        args.clusters = len(args.init_sample_ids)
    if not 1 <= args.clusters <= LABELS_MAX:
        parser.error("-k takes 1 to %d groups (got %d)" % (LABELS_MAX, args.clusters))
    _check_within_without(parser, args)
    _refuse_shards(parser, args, CLUSTER_SHARDS_REFUSAL)


def _check_pca_flags(parser, args):
    """`pca`: the numbers of the fit, what --axes leaves no room for, one query source at most, the files read.  Leaves the
    labels in args.label_groups (None without --labels) and the restriction's parts where _check_restriction_flags leaves
    them."""
    from .junctions import parse_groups_file
    from .search import PCA_MAX_BLOCK, PCA_MAX_COMPONENTS, PCA_SHARDS_REFUSAL, pca_width_refusal
    fit_flags = (("-p/--components", _given(args, "components")), ("--extra", _given(args, "extra")), ("--no-center", args.no_center),
                 ("--seed", _given(args, "seed")), ("--tolerance", _given(args, "tolerance")),
                 ("--max-iterations", _given(args, "max_iterations")), ("--within", args.within is not None),
                 ("--without", args.without is not None), ("--save-axes", args.save_axes is not None))
    if args.axes is not None:
        _refuse(parser, "--axes cannot be used with %s: the axes are read from the file and nothing is fitted", fit_flags)
    if not 1 <= args.components <= PCA_MAX_COMPONENTS or args.extra < 0 or args.components + args.extra > PCA_MAX_BLOCK:
        parser.error(pca_width_refusal(args.components, args.extra))
    if args.seed < 0:
        parser.error("--seed takes a number >= 0 (got %d)" % args.seed)
    if not (args.tolerance >= 0.0) or args.tolerance == float("inf"):
        parser.error("--tolerance takes a finite number >= 0 (got %r)" % args.tolerance)
    if args.max_iterations < 1:
        parser.error("--max-iterations takes a positive number (got %d)" % args.max_iterations)
    if args.format is not None and args.format not in ("sam", "bed", "raw"):
        parser.error("-f takes one of sam, bed, raw (got %r)" % args.format)
    if args.format is not None and args.intropolis is not None:
        parser.error("pca takes one query source: --intropolis or a stream on stdin with -f (got both)")
    if args.summary_only and args.output is not None:
        parser.error("--summary-only and -o cannot be used together: -o takes the lines --summary-only leaves out")
    args.query_id = args.query_ids = args.leave_out_groups = None
    args.label_groups = _read_file(parser, parse_groups_file, args.labels)
    if args.labels is not None and not args.label_groups:
        parser.error("--labels %s names no label" % args.labels)
    _read_restriction(parser, args, groups=False)
    _check_within_without(parser, args)
    _refuse_shards(parser, args, PCA_SHARDS_REFUSAL)


def _check_downsample_flags(parser, args):
    """--downsample: `search` and `recovery`, by item only, with the file that names the lines unless --unhashed; --lost-only
    and --downsample-seed only with it.  Leaves the rates in args.downsample_parts."""
    args.downsample_parts = None
    if args.downsample is None:
        _refuse(parser, "%s cannot be used without --downsample",
                (("--lost-only", getattr(args, "lost_only", False)), ("--downsample-seed", _given(args, "downsample_seed"))))
        return
    if args.subparser_name == 'junctions':
        parser.error("--downsample cannot be used with junctions")
    _refuse(parser, "--downsample cannot be used with %s",
            [("--intropolis", args.intropolis is not None), ("--supersamples", args.supersamples is not None)] + _stream_flags(args)
            + [("--results-sweep", getattr(args, "results_sweep", None) is not None)])
    if args.query_id is None and args.query_ids is None:
        parser.error("--downsample thins samples of the index: it needs -q or --query-ids, not a query from a stream")
    junction_file = args.junction_file if args.subparser_name == 'recovery' else args.unhashed_junction_file
    if junction_file is None and not args.unhashed:
        parser.error("--downsample needs --junction-file, the intropolis file the index was made from (unless --unhashed)")
    from .junctions import parse_downsample
    try:
        args.downsample_parts = parse_downsample(args.downsample)
    except ValueError as e:
        parser.error("--downsample takes 1 to 16 distinct comma-separated rates in [0, 1], such as 0.5,0.1,0.01 (%s)" % e)


def _check_restriction_flags(parser, args):
    """--within / --without / --leave-out-groups: the files read and checked against each other and against the query
    kind.  Leaves the ids in args.within_ids / args.without_ids and the groups in args.leave_out (None where the flag is
    absent), and args.restriction = None for main() to fill in."""
    args.within_ids = args.without_ids = args.leave_out = args.restriction = None
    if args.within is None and args.without is None and args.leave_out_groups is None:
        return
    _refuse(parser, "--within, --without and --leave-out-groups cannot be used with %s", _stream_flags(args))
    _read_restriction(parser, args)
    _check_within_without(parser, args)
    if args.leave_out is not None:
        why = "it takes queries that are samples of the index (-q, --query-ids, --downsample)"
        _refuse(parser, "--leave-out-groups cannot be used with %s",
                (("--intropolis", args.intropolis is not None, why), ("--supersamples", args.supersamples is not None, why),
                 ("--unhashed", args.unhashed, why),
                 ("a query from a stream", args.query_id is None and args.query_ids is None, why)))


def _check_supersample_flags(parser, args):
    """--supersamples: `search` only, with the file that names the lines and without another query."""
    if args.supersamples is None:
        return
    if args.subparser_name != 'search':
        parser.error("--supersamples cannot be used with %s" % args.subparser_name)
    if args.unhashed_junction_file is None:
        parser.error("--supersamples needs --junction-file, the intropolis file the index was made from")
    _refuse(parser, "--supersamples cannot be used with %s",
            [("-q/--query-id", args.query_id is not None), ("--query-ids", args.query_ids is not None),
             ("--intropolis", args.intropolis is not None)] + _stream_flags(args))


def _check_recovery_flags(parser, args):
    """`recovery`: the grid, the flags that make no sense here, and a query that names its truth."""
    from .junctions import parse_recovery_grid
    try:
        args.grid_parts = parse_recovery_grid(args.grid)
    except ValueError as e:
        parser.error("--grid takes <frequencies>:<coverages>, such as 0,.05,.5:1,5,50, with at most 15 coverages (%s)" % e)
    args.sweep = None
    if args.results_sweep is not None:
        from .junctions import parse_results_sweep
        try:
            args.sweep = parse_results_sweep(args.results_sweep)
        except ValueError as e:
            parser.error("--results-sweep takes at most 8 comma-separated result counts, each 1 to 64, such as 5,10,20 (%s)" % e)
        if args.sweep[-1] > args.results:
            parser.error("--results-sweep %d is more than -r %d: the counts are prefixes of the one search -r deep"
                         % (args.sweep[-1], args.results))
    _refuse(parser, "%s cannot be used with recovery",
            _stream_flags(args) + [("-m/--metadata", args.metadata), ("-d/--distances", args.distances), ("--unhashed", args.unhashed)])
    if args.query_id is None and args.query_ids is None and args.intropolis is None:
        parser.error("recovery needs a query whose true junctions are known: -q, --query-ids, or --intropolis with --truth")
    if args.intropolis is not None and (args.truth is None or args.junction_file is None):
        parser.error("recovery --intropolis needs --truth, the file with the true junctions of the same samples, and "
                     "--junction-file, the intropolis file the index was made from")
    if args.truth is not None and args.intropolis is None:
        parser.error("--truth cannot be used without --intropolis")


def _check_use_trees_flags(parser, args):
    """search --use-trees: the approximate, unrestricted, hashed search only."""
    if _use_trees(args) is None:
        return
    if args.use_trees < 1:
        parser.error("--use-trees takes a positive tree count (got %d)" % args.use_trees)
    _refuse(parser, "--use-trees cannot be used with %s",
            (("-e/--exact", args.exact), ("--unhashed", args.unhashed), ("--within", args.within is not None),
             ("--without", args.without is not None), ("--leave-out-groups", args.leave_out_groups is not None)))


def _check_recall_flags(parser, args):
    """`recall`: exactly one query source, the two lists (`all` is resolved once the index is read), -r within the limit."""
    from .search import RECALL_MAX_K, parse_int_list
    _check_sources(parser, args, "recall", ("query_id", "query_ids", "intropolis", "sample"), stream=False)
    if not 1 <= args.results <= RECALL_MAX_K:
        parser.error("-r %d: recall compares 1 to %d results" % (args.results, RECALL_MAX_K))
    try:
        parse_int_list(args.trees, "--trees", all_value=1 << 30)      # (checked again with the index's tree count)
        args.search_k_list = parse_int_list(args.search_ks, "--search-ks")
    except ValueError as e:
        parser.error("--trees and --search-ks take comma-separated positive integers in ascending order, at most 64, such as "
                     "10,20,50 (%s)" % e)


def _check_hashing_flags(parser, args):
    """`hashing`: the flags of `search` that make no sense here, exactly one query source, -r within the limit and the
    --features list (`index` is resolved once the index is read)."""
    from .search import RECALL_MAX_K, parse_features_list
    population = "the population is the index's items at every width"
    _refuse(parser, "hashing cannot be used with %s",
            (("-e/--exact", args.exact, "every width is searched exactly already; --n-trees adds the forest search"),
             ("--unhashed", args.unhashed, "the unhashed search is the truth every width is compared with"),
             ("--within", args.within is not None, population), ("--without", args.without is not None, population),
             ("--leave-out-groups", args.leave_out_groups is not None, population),
             ("--intropolis", args.intropolis is not None,
              "the queries are samples of the index, whose rows the junction store holds: name them with -q, --query-ids or "
              "--sample")))
    _check_sources(parser, args, "hashing", ("query_id", "query_ids", "sample"), stream=False)
    if not 1 <= args.results <= RECALL_MAX_K:
        parser.error("-r %d: hashing compares 1 to %d results" % (args.results, RECALL_MAX_K))
    if args.n_trees is None and _given(args, "search_k"):
        parser.error("--search-k cannot be used without --n-trees")
    if args.n_trees is not None and args.n_trees < 1:
        parser.error("--n-trees takes a positive tree count (got %d)" % args.n_trees)
    if args.search_k < 1:
        parser.error("--search-k takes a positive number (got %d)" % args.search_k)
    try:
        tokens = [t.strip() for t in args.features.split(",")]
        if tokens.count("index") > 1:
            raise ValueError("--features: 'index' is named twice")
        rest = [t for t in tokens if t != "index"]
        if len(tokens) > 16:
            raise ValueError("--features: %d entries, at most 16 are taken" % len(tokens))
        if rest:
            parse_features_list(",".join(rest))           # (checked again, in place, with the index's width)
    except ValueError as e:
        parser.error("--features takes comma-separated widths in ascending order, at most 16, each 1 to 32768 or the word "
                     "index, such as 500,3000,index (%s)" % e)


def _check_labels_flags(parser, args, command='labels'):
    """`labels` (and `mixture`, which takes the same queries and files; more labels than it takes is its own ValueError): at
    most one named query source (none: a stream on stdin), the files read and checked against each other and
    against the query kind.  Leaves the labels in args.label_groups and the restriction's parts where
    _check_restriction_flags leaves them."""
    from .junctions import parse_groups_file
    from .search import LABELS_MAX, labels_max_refusal
    given = _check_sources(parser, args, command, ("query_id", "query_ids", "sample", "all_items", "intropolis"), stream=True)
    if args.top < 1:
        parser.error("--top takes a positive number of labels (got %d)" % args.top)
    args.external = args.intropolis is not None or not given
    source = "--intropolis" if args.intropolis is not None else "a query from a stream"
    if args.external and args.matrix:
        parser.error("--matrix cannot be used with %s: the label map compares the queries' own labels, and only a sample of "
                     "the index has one (-q, --query-ids, --sample, --all)" % source)
    if args.external and args.leave_out_groups is not None:
        parser.error("--leave-out-groups cannot be used with %s: it takes queries that are samples of the index "
                     "(-q, --query-ids, --sample, --all)" % source)
    args.label_groups = _read_file(parser, parse_groups_file, args.labels)
    _read_restriction(parser, args)
    if not args.label_groups:
        parser.error("--labels %s names no label" % args.labels)
    if command == 'labels' and len(args.label_groups) > LABELS_MAX:
        parser.error(labels_max_refusal(len(args.label_groups)))
    _check_within_without(parser, args)


def _check_mixture_flags(parser, args):
    """`mixture`: the flags of the searches that make no sense here and the numbers of the fit, then what `labels` checks."""
    _refuse(parser, "mixture cannot be used with %s",
            (("-e/--exact", args.exact, "the fit is made in fp64 already"),
             ("--unhashed", args.unhashed, "the centroids are sums of the index's rows, in the hashed space"),
             ("--leave-out-groups", args.leave_out_groups is not None,
              "a query that is a sample of the index is left out of its own label's centroid, nothing else is"),
             ("--supersamples", args.supersamples is not None,
              "pool the samples with `morna supersample` and feed its file on stdin with -f raw")))
    if not (args.min_share >= 0.0 and args.min_share <= 1.0):
        parser.error("--min-share takes a share, 0 to 1 (got %r)" % args.min_share)
    if not (args.tolerance >= 0.0) or args.tolerance == float("inf"):
        parser.error("--tolerance takes a finite number >= 0 (got %r)" % args.tolerance)
    if args.max_sweeps < 1:
        parser.error("--max-sweeps takes a positive number of sweeps (got %d)" % args.max_sweeps)
    _check_labels_flags(parser, args, command='mixture')


def _check_explain_flags(parser, args):
    """`explain`: at most one named query source (none: a stream on stdin), the numbers, what --against excludes, and the
    files the command cannot do without.  Leaves the ids of --against in args.against_ids and the restriction's parts where
    _check_restriction_flags leaves them."""
    from .junctions import MAX_NEAREST
    given = _check_sources(parser, args, "explain", ("query_id", "query_ids", "sample", "intropolis"), stream=True)
    if args.top < 1 or args.top > 64:
        parser.error("--top takes 1 to 64 junctions per pair (got %d)" % args.top)
    if args.results < 1 or args.results > MAX_NEAREST:
        parser.error("-r takes 1 to %d results (got %d)" % (MAX_NEAREST, args.results))
    args.external = not given or args.intropolis is not None
    args.against_ids = None
    if args.against is not None:
        why = "no search runs, the samples it lists are the results"
        _refuse(parser, "--against cannot be used with %s",
                (("-r/--results", _given(args, "results"), why), ("-e/--exact", args.exact, why), ("--unhashed", args.unhashed, why),
                 ("--search-k", _given(args, "search_k"), why), ("--within", args.within is not None, why),
                 ("--without", args.without is not None, why)))
        args.against_ids = _parse_ids(parser, args.against, "--against")
        if len(args.against_ids) > MAX_NEAREST:
            parser.error("--against takes at most %d samples (got %d)" % (MAX_NEAREST, len(args.against_ids)))
    if args.unhashed:
        _refuse(parser, "--unhashed cannot be used with %s", (("-e/--exact", args.exact), ("--search-k", _given(args, "search_k"))))
    _read_restriction(parser, args, groups=False)
    _check_within_without(parser, args)
    _refuse_shards(parser, args, "explain is not available on an index of row shards (.shards.mor, one process per shard, "
                   "--device a,b): run it on an index built without --shards")
    _require_store(args, weights=True, parser=parser)


def _check_batch_flags(parser, args):
    """--intropolis / --query-ids exclude each other and the single-query flags."""
    batch = [flag for flag, on in (("--intropolis", args.intropolis is not None), ("--query-ids", args.query_ids is not None)) if on]
    if not batch:
        return
    if len(batch) > 1:
        parser.error("--intropolis and --query-ids cannot be used together")
    _refuse(parser, batch[0] + " cannot be used with %s", [("-q/--query-id", args.query_id is not None)] + _stream_flags(args))
    if args.query_ids is not None:
        args.query_ids = _parse_ids(parser, args.query_ids)


def _check_unhashed_flags(parser, args):
    """--unhashed: `search` only, without the flags of the hashed searches; a query from outside the index needs the file
    that names the lines."""
    if not args.unhashed:
        return
    if args.subparser_name == 'junctions':
        parser.error("--unhashed cannot be used with junctions")
    _refuse(parser, "--unhashed cannot be used with %s",
            [("-e/--exact", args.exact)] + _stream_flags(args) + [("--search-k", _given(args, "search_k"))])
    if args.query_id is None and args.query_ids is None and args.unhashed_junction_file is None:
        parser.error("--unhashed with a query from %s needs --junction-file, the intropolis file the index was made from"
                     % ("--intropolis" if args.intropolis is not None else "a stream"))


def _check_junction_flags(parser, args):
    """`junctions`: the filter's two parts, what the result limit allows, and the flags that make no sense here."""
    from .junctions import parse_junction_filter
    try:
        args.junction_filter_parts = parse_junction_filter(args.junction_filter)
    except ValueError:
        parser.error("--junction-filter takes <proportion>,<coverage>, such as .05,5 (got %r)" % args.junction_filter)
    _refuse(parser, "%s cannot be used with junctions", _stream_flags(args))


def _searching(args, stdin, stdout):
    """`search`, `junctions` and `recovery`: the searcher of the index, over several devices or with one process per shard
    where the index has shards, its restriction, and the command on it."""
    import os
    from .search import MornaSearch
    devices = [int(d) for d in str(args.device).split(',')]
    on_shards, world = _shards(args)
    rank = int(os.environ.get("RANK", "0"))
    dist = None
    pooling = args.subparser_name in ('junctions', 'recovery')
    sharded = world > 1 and on_shards
    if sharded and (pooling or args.unhashed or args.supersamples is not None or args.downsample is not None
                    or _use_trees(args) is not None):
        raise RuntimeError(_ONE_PROCESS_REFUSAL)
    if pooling:
        from .junctions import MAX_RESULTS
        if args.results > MAX_RESULTS:
            raise ValueError("-r %d: junctions takes at most %d results (found_in is one 64-bit word per junction)"
                             % (args.results, MAX_RESULTS))
    if pooling or args.downsample is not None:
        _require_store(args)
    if sharded:
        # torchrun with one process per shard: every rank runs this function with the same query (rank 0 reads the stream
        # and hands it over) and calls the same collectives; rank 0 prints
        import io
        import torch
        import torch.distributed as dist
        from ._lib import device_count
        n_dev = device_count()
        local = int(os.environ.get("LOCAL_RANK", "0"))
        backend = "nccl" if n_dev >= int(os.environ.get("LOCAL_WORLD_SIZE", str(world))) else "gloo"   # RCCL wants a GPU per rank
        torch.cuda.set_device(local % n_dev)
        dist.init_process_group(backend, rank=rank, world_size=world)
        searcher = MornaSearch(basename=args.basename, device=local % n_dev, rank=rank, world=world)
        if rank != 0:
            stdout = io.StringIO()
    else:
        searcher = MornaSearch(basename=args.basename, device=devices if len(devices) > 1 else devices[0])
    try:
        args.restriction = _make_restriction(args, searcher)
        if args.supersamples is not None:
            return _search_supersamples(args, searcher, stdout)
        if args.downsample is not None and args.subparser_name == 'search':
            return _search_downsample(args, searcher, stdout)
        if args.unhashed:
            return _search_unhashed(args, searcher, stdin, stdout)
        if args.subparser_name == 'junctions':
            return _junctions(args, searcher, stdin, stdout)
        if args.subparser_name == 'recovery':
            return _recovery(args, searcher, stdin, stdout)
        return _search(args, searcher, stdin, stdout, dist, rank)
    finally:
        if dist is not None:
            searcher.annoy_index.close()
            dist.destroy_process_group()


# ---- what the flags mean once an index is open ------------------------------------------------------------------------------------
def _make_restriction(args, searcher):
    """The searcher's restriction of the three flags (None without them), its one line on stderr.  Every query sample the
    groups file does not name becomes a group of its own."""
    if args.within_ids is None and args.without_ids is None and args.leave_out is None:
        return None
    groups = None
    if args.leave_out is not None:
        groups = list(args.leave_out)
        named = set(i for _, ids in groups for i in ids)
        query_ids = args.query_ids if isinstance(args.query_ids, list) else ([args.query_id] if args.query_id is not None else [])
        for query_id in query_ids:
            if query_id not in named and query_id in searcher.internal_id_map:
                groups.append(("query-%d" % query_id, [query_id]))
                named.add(query_id)
    restriction = searcher.restriction(args.within_ids, args.without_ids, groups)
    sys.stderr.write(restriction.summary() + "\n")
    return restriction


def _restriction(args):
    """The restriction main() made of the three flags; None without them (and for a caller that made `args` itself)."""
    return getattr(args, "restriction", None)


def _leaves_out(args):
    """--leave-out-groups was given: the search itself leaves the query out."""
    return getattr(args, "leave_out", None) is not None


def _search_k(args):
    """--search-k as given; without it the command's default of 100, or under an allow-list -1: the searcher then scales
    annoy's default by the share of the index that is allowed (search.restricted_search_k)."""
    r = _restriction(args)
    if r is not None and r.allow is not None and not _given(args, "search_k"):
        return -1
    return args.search_k


def _use_trees(args):
    """search --use-trees; None without it (and for `junctions` / `recovery`, which do not take it)."""
    return getattr(args, "use_trees", None)


def _max_distance(args):
    """search --max-distance; None without it (and for the commands that do not take it)."""
    return getattr(args, "max_distance", None)


def _radius_cap(args):
    """-r under --max-distance: a cap when it was given on the command line, None otherwise."""
    return args.results if _given(args, "results") else None


def _single(args):
    """The MornaSearch of a command that runs on one device."""
    from .search import MornaSearch
    return MornaSearch(basename=args.basename, device=int(str(args.device).split(',')[0]))


def _open_single(args, refusal, world=None, weights=None):
    """_single() for a command that refuses shards once it runs: RuntimeError under WORLD_SIZE > 1 (or `world`, the
    exception of a command that words it otherwise), ValueError(refusal) on an index of row shards; weights: the junction
    store, and with True its weights, must be there too."""
    on_shards, processes = _shards(args)
    if processes > 1:
        raise world or RuntimeError(_ONE_PROCESS_REFUSAL)
    if on_shards:
        raise ValueError(refusal)
    if weights is not None:
        _require_store(args, weights=weights)
    return _single(args)


def _query_sample_ids(args, searcher, check=True):
    """-q / --query-ids / --sample / --all as sample ids; check: every one is a sample of the index (`hashing` leaves that to
    hashing_sweep)."""
    all_items = getattr(args, "all_items", False)
    if all_items or getattr(args, "sample", None) is not None:
        import numpy as np
        n = searcher.annoy_index.get_n_items()
        inv = searcher._inverse_map()
        if not all_items and args.sample > n:
            raise ValueError("--sample %d: the index holds %d samples" % (args.sample, n))
        picked = range(n) if all_items else np.random.RandomState(args.sample_seed).choice(n, size=args.sample, replace=False)
        ids = [inv[int(i)] for i in picked]
    else:
        ids = args.query_ids if args.query_ids is not None else [args.query_id]
    for query_id in ids if check else ():
        if query_id not in searcher.internal_id_map:
            raise ValueError("Querying sample id " + str(query_id)
                             + " is not possible because no internal id is mapped to that "
                             + "sample id. Likely no sample with that id was included "
                             + "in the index.")
    return ids


def _stream_parser(fmt):
    """The generator of junctions for -f sam / bed / raw."""
    from . import streams
    return {"sam": streams.junctions_from_sam_stream, "bed": streams.junctions_from_bed_stream,
            "raw": streams.junctions_from_raw_stream}[fmt]


def _hash_stream(searcher, junctions):
    """A stream as the searcher's hashed query: the junctions the index knows, then finalize_query."""
    for junction in junctions:
        if " ".join(str(_) for _ in junction[:3]) in searcher.sample_frequencies:
            searcher.update_query(junction)
    searcher.finalize_query()


def _stream_coverage(junctions):
    """A stream's coverage summed per junction, as update_query sums it."""
    coverage = {}
    for junction in junctions:
        key = " ".join(str(_) for _ in junction[:3])
        coverage[key] = coverage.get(key, 0) + int(junction[3])
    return coverage


def _batch_search(args, searcher, batch, n_results, distances=None, **query_groups):
    """The radius (--max-distance), exact (-e) or approximate search of a batch of hashed queries with the command's flags;
    query_groups: the group every query carries, from the caller whose queries have one.  The radius form takes no n_trees."""
    common = dict(include_distances=args.distances if distances is None else distances, meta_db=args.metadata,
                  restriction=_restriction(args), **query_groups)
    if _max_distance(args) is not None:
        return searcher.exact_radius_nn_batch(batch, _max_distance(args), num_neighbors=_radius_cap(args), **common)
    if args.exact:
        return searcher.exact_search_nn_batch(batch, n_results, **common)
    return searcher.search_nn_batch(batch, n_results, _search_k(args), n_trees=_use_trees(args), **common)


def _unhashed_search(args, searcher, terms, n_results, distances=None):
    """The unhashed search of a batch of queries given as term lists, with the command's flags."""
    return searcher.unhashed_search_nn_batch(terms, n_results, include_distances=args.distances if distances is None else distances,
                                             meta_db=args.metadata, restriction=_restriction(args))


def _write_blocks(stdout, labels, results, header, collect=None):
    """One block per query: header(label), then the result lines or "# error: ..."; 1 when some query failed."""
    from .search import results_output
    failed = False
    for label, res in zip(labels, results):
        header(label)
        if isinstance(res, Exception):
            stdout.write("# error: %s\n" % res)
            failed = True
        else:
            results_output(res, stdout)
            if collect is not None:
                collect.append((label, res))
    return 1 if failed else 0


def _write_member_header(stdout, query_id, internal_id, numbered):
    """A by-sample query's "# query" line (in a batch) and search_member_n's two lines."""
    if numbered:
        stdout.write("# query %d\n" % query_id)
    stdout.write("querying by sample id " + str(query_id) + "\n")
    stdout.write("this is internal id " + str(internal_id) + "\n")


# ---- the commands -----------------------------------------------------------------------------------------------------------------
def _index(args, stdin, stdout):
    import os
    from .index import go_index
    rank, device = None, int(str(args.device).split(',')[0])
    if args.shards > 1 and int(os.environ.get("WORLD_SIZE", "1")) == args.shards:   # one process per GPU
        from ._lib import device_count
        rank = int(os.environ.get("RANK", "0"))
        device = int(os.environ.get("LOCAL_RANK", "0")) % device_count()   # (fewer GPUs than ranks: the ranks share them)
    go_index(args.intropolis, args.basename, args.features, args.n_trees, args.sample_count,
             args.sample_threshold, args.buffer_size, args.verbose, args.metafile, device=device,
             native=not args.python_parse, cache=args.cache, shards=args.shards, rank=rank,
             junction_store=args.junction_store)
    return 0


def _recall(args, stdin, stdout):
    """`recall`: one exact search and one sweep over --trees x --search-ks on the GPU; a block per query and the table over
    all of them."""
    from .search import TREES_SHARDS_REFUSAL, format_recall_rows, parse_int_list
    searcher = _open_single(args, TREES_SHARDS_REFUSAL)
    n_trees = searcher.annoy_index.get_n_trees()
    trees = parse_int_list(args.trees, "--trees", all_value=n_trees)
    if trees[-1] > n_trees:
        raise ValueError("--trees %d: the index has %d trees" % (trees[-1], n_trees))
    if args.intropolis is not None:
        batch = searcher.queries_from_intropolis(args.intropolis)
        labels, queries = batch.ext_ids, batch
    else:
        labels = _query_sample_ids(args, searcher)
        queries = [searcher.internal_id_map[query_id] for query_id in labels]
    table = searcher.search_recall(queries, args.results, trees, args.search_k_list)
    if not args.summary_only:
        for q, label in enumerate(labels):
            stdout.write("# query %s\n" % label)
            stdout.write(format_recall_rows(table.rows(q)))
    rows, failed = table.summary()
    stdout.write("# all %d queries\n" % len(labels))
    stdout.write(format_recall_rows(rows))
    if failed > 0:
        stdout.write("# exact search failed for %d queries\n" % failed)
    return 0


def _hashing(args, stdin, stdout):
    """`hashing`: the unhashed neighbours of the queries once, then for every width of --features the index's items hashed
    again from the junction store and searched on the GPU; a block per query and the table over all of them."""
    from .search import HASHING_SHARDS_REFUSAL, format_hashing_rows, parse_features_list
    searcher = _open_single(args, HASHING_SHARDS_REFUSAL, weights=True)
    dims = parse_features_list(args.features, index_dim=searcher.dim)
    labels = _query_sample_ids(args, searcher, check=False)
    table = searcher.hashing_sweep(labels, args.results, dims, args.junction_file, n_trees=args.n_trees,
                                   search_k=args.search_k if args.n_trees is not None else None)
    if not args.summary_only:
        for q, label in enumerate(labels):
            stdout.write("# query %s\n" % label)
            stdout.write(format_hashing_rows(table.rows(q)))
    stdout.write("# all %d queries\n" % len(labels))
    stdout.write(format_hashing_rows(table.summary()))
    return 0


def _label_queries(args, searcher, stdin):
    """The queries of `labels` and `mixture` from their flags: (queries as MornaSearch.label_separation takes them, the ids
    printed for them)."""
    if args.intropolis is not None:
        queries = searcher.queries_from_intropolis(args.intropolis)
        return queries, queries.ext_ids
    if args.external:                                          # a stream: one query, as `search` makes it
        import numpy as np
        _hash_stream(searcher, _stream_parser(args.format)(stdin))
        return np.array([searcher.query_sample], dtype=np.float64), ["stdin"]
    ids = _query_sample_ids(args, searcher)
    args.query_ids = list(ids)                                 # (a query the groups file does not name is a group of its own)
    return [searcher.internal_id_map[query_id] for query_id in ids], ids


def _mixture(args, stdin, stdout):
    """`mixture`: every query fitted on the GPU as a non-negative blend of the label centroids; a block per query, the table
    over all of them and, with --matrix, the table of mean shares."""
    from .search import MIXTURE_LABELS_MAX, MIXTURE_SHARDS_REFUSAL, format_label_rows, mixture_max_refusal
    if len(args.label_groups) > MIXTURE_LABELS_MAX:
        raise ValueError(mixture_max_refusal(len(args.label_groups)))
    searcher = _open_single(args, MIXTURE_SHARDS_REFUSAL)
    queries, ids = _label_queries(args, searcher, stdin)
    args.restriction = _make_restriction(args, searcher)
    table = searcher.label_mixture(queries, args.label_groups, restriction=args.restriction, tol=args.tolerance,
                                   max_sweeps=args.max_sweeps)
    if not args.summary_only:
        for q, query_id in enumerate(ids):
            stdout.write(table.header(q, query_id))
            stdout.write(format_label_rows(table.rows(q, args.top, args.min_share)))
    rows, without = table.summary(args.min_share)
    stdout.write("# all %d queries\n" % len(ids))
    stdout.write(format_label_rows(rows))
    if without > 0:
        stdout.write("# %d queries without %s\n" % (without, "a positive weight" if args.external else "a label of their own"))
    if args.matrix:
        stdout.write("# share matrix\n")
        stdout.write(format_label_rows([(name,) + tuple(row) for name, row in zip(table.names, table.matrix())]))
    return 0


def _labels(args, stdin, stdout):
    """`labels`: one scan of the index on the GPU that keeps, per query and label, the sum of the distances and their number;
    a block per query, the table over all of them and, with --matrix, the label map."""
    from .search import LABELS_SHARDS_REFUSAL, format_label_rows
    searcher = _open_single(args, LABELS_SHARDS_REFUSAL)
    queries, ids = _label_queries(args, searcher, stdin)
    args.restriction = _make_restriction(args, searcher)
    table = searcher.label_separation(queries, args.label_groups, restriction=args.restriction)
    if not args.summary_only:
        for q, query_id in enumerate(ids):
            stdout.write("# query %s\tlabel %s\n" % (query_id, table.own_name(q) or "-"))
            stdout.write(format_label_rows(table.rows(q, args.top)))
    rows, without = table.summary()
    stdout.write("# all %d queries\n" % len(ids))
    stdout.write(format_label_rows(rows))
    if without > 0:
        stdout.write("# %d queries without a %s\n" % (without, "labelled sample to compare with" if args.external else "silhouette"))
    if args.matrix:
        stdout.write("# label map\n")
        stdout.write(format_label_rows([(name,) + tuple(row) for name, row in zip(table.names, table.map())]))
    return 0


def _by_label(labels, ext_ids, found):
    """The results of a batch of the hashed searches (sample ids ext_ids) in the order of `labels`."""
    by_id = dict(zip(ext_ids, found))
    return [by_id.get(label, ValueError("sample %s holds no junction of the index" % label)) for label in labels]


def _explain_searches(args, searcher, stream, terms, query_ids, labels):
    """The searches of `explain` without --against: what `search` runs with the same flags, distances included; one result
    tuple (or exception) per query."""
    if query_ids is not None and args.unhashed:
        return searcher.unhashed_search_member_n_batch(query_ids, args.results, include_distances=True, meta_db=args.metadata,
                                                       restriction=_restriction(args))
    if query_ids is not None:
        return searcher.search_member_n_batch(query_ids, args.results, _search_k(args), include_distances=True,
                                              meta_db=args.metadata, restriction=_restriction(args))[1]
    if args.unhashed:
        return _unhashed_search(args, searcher, terms, args.results, distances=True)
    if args.intropolis is not None:
        batch = searcher.queries_from_intropolis(args.intropolis)
        return _by_label(labels, batch.ext_ids, _batch_search(args, searcher, batch, args.results, distances=True))
    _hash_stream(searcher, stream)
    if args.exact:
        return [searcher.exact_search_nn(args.results, include_distances=True, meta_db=args.metadata, restriction=_restriction(args))]
    return [searcher.search_nn(args.results, _search_k(args), include_distances=True, meta_db=args.metadata,
                               restriction=_restriction(args))]


def _explain_against(args, searcher, stream, query_ids, labels):
    """explain --against: no search; every query gets the listed samples in the order listed, each with its distance in
    the exact search restricted to them."""
    import numpy as np
    from .metadb import lookup_meta
    for sample_id in args.against_ids:
        if sample_id not in searcher.internal_id_map:
            raise ValueError("--against names sample id %d, which is not a sample of the index" % sample_id)
    listed = [searcher.internal_id_map[s] for s in args.against_ids]
    restriction = searcher.restriction(within=sorted(set(args.against_ids)))
    n = len(set(listed))
    if query_ids is not None:
        ids, d, cnt = searcher.annoy_index.exact_search_restricted(
            restriction.handle, n, items=np.array([searcher.internal_id_map[q] for q in query_ids], np.int32))
        found = searcher._batch_results(ids, d, cnt, True, False)
    elif args.intropolis is not None:
        batch = searcher.queries_from_intropolis(args.intropolis)
        found = _by_label(labels, batch.ext_ids, searcher.exact_search_nn_batch(batch, n, include_distances=True,
                                                                                restriction=restriction))
    else:
        _hash_stream(searcher, stream)
        found = [searcher.exact_search_nn(n, include_distances=True, restriction=restriction)]
    meta = lookup_meta(searcher.basename, list(args.against_ids)) if args.metadata else None
    results = []
    for res in found:
        if isinstance(res, Exception):
            results.append(res)
            continue
        distance = dict(zip(res[0], res[1]))
        results.append((listed, [distance.get(i, float("nan")) for i in listed]) + ((meta,) if meta is not None else ()))
    return results


def _explain(args, stdin, stdout):
    """`explain`: the search of `search` with the same flags (or the samples of --against), then every (query, result) pair
    explained in one call on the GPU; a block per query, a line per pair and under it a line per junction of its top
    list."""
    from .junctions import (explain_rows, format_explain_rows, intropolis_query_terms, key_lines, line_names, query_terms)
    searcher = _single(args)
    store, w = searcher.unhashed_store()
    stream, terms, query_ids = None, None, None
    if args.intropolis is not None:
        labels, terms = intropolis_query_terms(args.intropolis, key_lines(args.junction_file, store.n_lines), w)
    elif args.external:                                        # a stream: one query, its coverages summed per junction
        stream = list(_stream_parser(args.format)(stdin))
        labels, terms = ["stdin"], [query_terms(_stream_coverage(stream), key_lines(args.junction_file, store.n_lines), w)]
    else:
        query_ids = _query_sample_ids(args, searcher)
        labels = list(query_ids)
    if args.against_ids is not None:
        results = _explain_against(args, searcher, stream, query_ids, labels)
    else:
        args.restriction = _make_restriction(args, searcher)
        results = _explain_searches(args, searcher, stream, terms, query_ids, labels)
    if len(results) != len(labels):
        raise RuntimeError("explain: %d queries, %d result lists" % (len(labels), len(results)))
    lists = [[] if isinstance(res, Exception) else list(res[0]) for res in results]
    rows = [store.sample(q) for q in query_ids] if query_ids is not None else terms
    explained = searcher.explain_results(lists, [searcher.internal_id_map[q] for q in query_ids] if query_ids is not None else terms,
                                         args.top)
    names = None
    if not args.summary_only:
        names = line_names(args.junction_file, [int(l) for pairs in explained for p in pairs for l in p.lines])
    inv = searcher._inverse_map()
    failed = False
    for label, res, pairs, (q_lines, q_cov) in zip(labels, results, explained, rows):
        stdout.write("# query %s\n" % label)
        if isinstance(res, Exception):
            stdout.write("# error: %s\n" % res)
            failed = True
            continue
        for rank, pair in enumerate(pairs):
            summary, top_rows = explain_rows(pair, q_lines, q_cov, w, names)
            stdout.write(format_explain_rows(rank + 1, res[0][rank], inv[int(res[0][rank])], res[1][rank], summary,
                                             () if args.summary_only else top_rows, res[2][rank] if args.metadata else None))
    return 1 if failed else 0


def _pairs(args, stdin, stdout):
    """`pairs`: one radius search by item over the whole index on the GPU, every sample bounded to the ids above its own; a
    line per pair, the summary line and, with --clusters, a line per connected component."""
    from .metadb import lookup_meta
    from .search import RADIUS_SHARDS_REFUSAL, format_cluster_line, format_pair_line, format_pairs_summary, pair_clusters
    searcher = _open_single(args, RADIUS_SHARDS_REFUSAL, world=ValueError(RADIUS_SHARDS_REFUSAL))
    args.restriction = _make_restriction(args, searcher)
    pairs = searcher.sample_pairs(args.max_distance, restriction=args.restriction)
    clusters = pair_clusters(pairs)
    if not args.summary_only:
        meta = {}
        if args.metadata:
            ids = sorted(set(i for p in pairs for i in p[:2]))
            # (a 1-tuple with the rest of the sample's metafile line, newline included, or None: metadb.lookup_meta)
            meta = dict((i, m[0].strip() if m else "-") for i, m in zip(ids, lookup_meta(args.basename, ids)))
        for a, b, d in pairs:
            stdout.write(format_pair_line(a, b, d, (meta[a], meta[b]) if args.metadata else None))
    n_samples = searcher.annoy_index.get_n_items() if args.restriction is None else args.restriction.n_allowed
    stdout.write(format_pairs_summary(n_samples, pairs, clusters))
    if args.clusters:
        for c in clusters:
            stdout.write(format_cluster_line(c))
    return 0


def _cluster(args, stdin, stdout):
    """`cluster`: spherical k-means over the index rows on the GPU; the header, a line per group, a line per sample and, with
    -o, the groups file."""
    from .metadb import lookup_meta
    from .search import write_groups_file
    searcher = _single(args)
    args.restriction = _make_restriction(args, searcher)
    clusters = searcher.cluster_samples(args.clusters, seed=args.seed, init_ids=args.init_sample_ids,
                                        max_iterations=args.max_iterations, restriction=args.restriction)
    meta = None
    if args.metadata:
        ids = [c for c in clusters.centres if c is not None]
        meta = dict((i, str(m)) for i, m in zip(ids, lookup_meta(args.basename, ids)))   # (as results_output prints an entry)
    stdout.write(clusters.header())
    stdout.write(clusters.rows(meta))
    if not args.summary_only:
        stdout.write(clusters.sample_lines())
    if args.output is not None:
        write_groups_file(args.output, clusters.groups)
    return 0


def _pca(args, stdin, stdout):
    """`pca`: the axes fitted on the GPU (or read with --axes); the header, a line per component, a line per indexed sample,
    with --labels the block of label means, and a line per query."""
    import numpy as np
    from .metadb import lookup_meta
    from .search import (PCA_SHARDS_REFUSAL, format_pca_label_means, format_pca_row, load_pca_axes, pca_label_means,
                         restriction_arrays, save_pca_axes)
    searcher = _open_single(args, PCA_SHARDS_REFUSAL)
    n, dim = searcher.annoy_index.get_n_items(), searcher.annoy_index.f
    names = item_label = None
    if args.label_groups is not None:
        names = [label for label, _ in args.label_groups]
        _, item_label, _ = restriction_arrays(searcher.internal_id_map, n, groups=args.label_groups)
    if args.axes is not None:
        pca = load_pca_axes(args.axes, dim)
    else:
        args.restriction = _make_restriction(args, searcher)
        pca = searcher.principal_axes(args.components, extra=args.extra, center=not args.no_center, seed=args.seed,
                                      tol=args.tolerance, max_iterations=args.max_iterations, restriction=args.restriction)
    if args.save_axes is not None:
        save_pca_axes(args.save_axes, pca, dim)
    stdout.write(pca.header())
    stdout.write(pca.components())
    if not args.summary_only or names is not None:
        searcher.pca_samples(pca)
    if not args.summary_only:
        labels = meta = None
        if names is not None:
            labels = dict((sample_id, names[l]) for sample_id, l in zip(pca.samples, item_label.tolist()) if l >= 0)
        if args.metadata:
            meta = dict((i, str(m)) for i, m in zip(pca.samples, lookup_meta(args.basename, pca.samples)))
        lines = pca.sample_lines(labels, meta)
        if args.output is not None:
            with open(args.output, "w") as fh:
                fh.write(lines)
        else:
            stdout.write(lines)
    if names is not None:
        stdout.write(format_pca_label_means(pca_label_means(names, item_label, pca.coords)))
    queries = ids = None
    if args.intropolis is not None:
        queries = searcher.queries_from_intropolis(args.intropolis)
        ids = queries.ext_ids
    elif args.format is not None:                              # a stream: one query, as `search` makes it
        _hash_stream(searcher, _stream_parser(args.format)(stdin))
        queries, ids = np.array([searcher.query_sample], dtype=np.float64), ["stdin"]
    if queries is not None:
        for query_id, row in zip(ids, searcher.pca_coordinates(pca, queries).tolist()):
            stdout.write(format_pca_row("# query %s" % query_id, row))
    return 0


def _junctions(args, searcher, stdin, stdout):
    """morna.py:1351-1353, 1486-1638: the search, printed as `search` prints it, then the junctions of every query's
    results filtered on the GPU in one call and written in one pass over --junction-file."""
    from .junctions import write_splice_files
    batch = args.intropolis is not None or args.query_ids is not None
    collected = []
    if not batch and args.query_id is None:
        args.format = "sam"                                    # morna.py:1352-1353
        with open(args.pass1_sam) as sam:
            rc = _search(args, searcher, sam, stdout, None, 0, collect=collected)
    else:
        rc = _search(args, searcher, stdin, stdout, None, 0, collect=collected)
    frequency_filter, coverage_filter = args.junction_filter_parts
    retained = searcher.retain_junctions([res[0] for _, res in collected], frequency_filter, coverage_filter)
    jobs = []
    for (label, res), kept in zip(collected, retained):
        stdout.write("Number of retained junctions: " + str(len(kept)) + "\n")      # morna.py:1573
        sys.stderr.write(str(len(kept)) + " junctions to begin with\n")             # morna.py:1586
        path = args.splicefile + "." + str(label) if batch else args.splicefile
        jobs.append((path, kept, searcher.result_sample_ids(res[0])))
    sys.stderr.flush()
    write_splice_files(args.junction_file, jobs)
    return rc


def _recovery(args, searcher, stdin, stdout):
    """The search of `search` (its result lines are not printed), then one histogram per query on the GPU and the tables
    of every (frequency, coverage) pair of the grid from it."""
    import contextlib
    import io
    from .junctions import format_recovery_rows, intropolis_truth, key_lines, recovery_rows, sum_recovery_rows
    if args.downsample is not None:
        return _recovery_downsample(args, searcher, stdout)
    frequencies, coverages = args.grid_parts
    wanted = args.results
    collected = []
    by_item = args.intropolis is None
    if by_item and not _leaves_out(args):
        args.results = wanted + 1                              # leave one out: the query is its own nearest neighbour
    # (--leave-out-groups: the search itself leaves the query's whole group out, the query included: exactly -r)
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):                     # (search_member_n prints its two lines itself)
        rc = _search(args, searcher, stdin, sink, None, 0, collect=collected)
    args.results = wanted
    labels = [label for label, _ in collected]
    extra = [0] * len(collected)
    if by_item:
        lists, truth = [], []
        for label, res in collected:
            own = searcher.internal_id_map[label]
            lists.append([i for i in res[0] if i != own][:wanted])
            truth.append(own)
        min_coverage = args.truth_coverage
    else:
        lists = [list(res[0])[:wanted] for _, res in collected]
        truth_of = intropolis_truth(args.truth, key_lines(args.junction_file, searcher.junction_store().n_lines), args.truth_coverage)
        truth = []
        for q, label in enumerate(labels):
            if label not in truth_of:
                raise ValueError("query sample %d of %s is not in %s: it has no truth" % (label, args.intropolis, args.truth))
            truth.append(truth_of[label][0])
            extra[q] = truth_of[label][1]
        sys.stderr.write("%d true junctions of %s are not in %s: they count as false negatives\n"
                         % (sum(extra), args.truth, args.junction_file))
        min_coverage = 1                                       # (intropolis_truth has applied --truth-coverage)
    if args.sweep is None:
        hist = searcher.junction_recovery(lists, truth, coverages, min_coverage) if lists else []
        slices = [(None, [hist[q] for q in range(len(lists))])]
    else:
        hist = searcher.junction_recovery_sweep(lists, truth, coverages, args.sweep, min_coverage) if lists else []
        slices = [(p, [hist[q][i] for q in range(len(lists))]) for i, p in enumerate(args.sweep)]
    tables = [[] for _ in slices]                              # per result count, per query
    for q, label in enumerate(labels):
        for i, (p, hists) in enumerate(slices):
            m = len(lists[q]) if p is None else min(p, len(lists[q]))
            rows = recovery_rows(hists[q], m, frequencies, coverages, extra_true=extra[q])
            tables[i].append(rows)
            if not args.summary_only:
                stdout.write("# query %s\tresults %d\ttrue %d\n" % (label, m, rows[0]["true_positive"] + rows[0]["false_negative"]))
                stdout.write(format_recovery_rows(rows))
    for i, (p, _) in enumerate(slices):
        stdout.write("# all %d queries%s\n" % (len(labels), "" if p is None else "\tresults %d" % p))
        stdout.write(format_recovery_rows(sum_recovery_rows(tables[i])))
    return rc


def _downsample_search(args, searcher, n_results, junction_file):
    """--downsample: every (query id, rate) a job, all jobs thinned in one call and searched in one batch.  Returns (jobs:
    (sample id, rate as typed) in the order (id given, rate typed), their junctions.Thinned, their results, an Exception
    instance where the reference's search would raise)."""
    ids = _query_sample_ids(args, searcher)
    typed, keep = args.downsample_parts
    jobs = [(query_id, t) for query_id in ids for t in typed]
    thinned = searcher.thin_samples([query_id for query_id, _ in jobs], keep * len(ids), args.downsample_seed)
    for (query_id, rate), row in zip(jobs, thinned):
        if len(row) == 0:
            sys.stderr.write("query %s at keep %s keeps no read: it is searched as a sample without junctions\n" % (query_id, rate))
    r = _restriction(args)
    own = None                                                 # every job carries its sample's group
    if r is not None and r.item_group is not None:
        own = r.own_groups([searcher.internal_id_map[query_id] for query_id, _ in jobs])
    if args.unhashed:
        return jobs, thinned, _unhashed_search(args, searcher, searcher.unhashed_terms_from_thinned(thinned), n_results)
    return jobs, thinned, _batch_search(args, searcher, searcher.queries_from_thinned(thinned, junction_file), n_results,
                                        query_groups=own)


def _search_downsample(args, searcher, stdout):
    """search --downsample: a block per (query id, rate), printed as --intropolis prints a sample's."""
    jobs, _, results = _downsample_search(args, searcher, args.results, args.unhashed_junction_file)
    return _write_blocks(stdout, jobs, results, lambda job: stdout.write("# query %d\tkeep %s\n" % job))


def _recovery_downsample(args, searcher, stdout):
    """recovery --downsample: the reference's downsample -> align -> recover experiment on the store.  Every (query id, rate)
    is searched with the thinned row, leave one out; the truth is the query's full row at --truth-coverage, or with
    --lost-only the lines of it the thinned row does not hold.  A job no search answers (no read kept, under -e) is tabulated
    with no results, named on stderr, and makes the return code 1, as `search --downsample` returns 1 for it."""
    from .junctions import format_recovery_rows, lost_lines, recovery_rows, sum_recovery_rows
    frequencies, coverages = args.grid_parts
    wanted = args.results
    jobs, thinned, results = _downsample_search(args, searcher, wanted + (1 if not _leaves_out(args) else 0), args.junction_file)
    typed = args.downsample_parts[0]
    store = searcher.junction_store()
    lists, truth, failed = [], [], False
    for (query_id, rate), row, res in zip(jobs, thinned, results):
        own = searcher.internal_id_map[query_id]
        if isinstance(res, Exception):
            sys.stderr.write("query %s at keep %s was not searched (%s): its table has no results\n" % (query_id, rate, res))
            failed = True
        found = [] if isinstance(res, Exception) else list(res[0])
        lists.append([i for i in found if i != own][:wanted])
        if args.lost_only:
            line, cov = store.sample(query_id)
            truth.append(lost_lines(line, cov, row.lines, args.truth_coverage))
        else:
            truth.append(own)
    hist = searcher.junction_recovery(lists, truth, coverages, args.truth_coverage) if lists else []
    tables = {rate: [] for rate in typed}
    for q, (query_id, rate) in enumerate(jobs):
        rows = recovery_rows(hist[q], len(lists[q]), frequencies, coverages)
        tables[rate].append(rows)
        if not args.summary_only:
            stdout.write("# query %s\tkeep %s\tresults %d\ttrue %d\n"
                         % (query_id, rate, len(lists[q]), rows[0]["true_positive"] + rows[0]["false_negative"]))
            stdout.write(format_recovery_rows(rows))
    for rate in typed:
        stdout.write("# all %d queries\tkeep %s\n" % (len(tables[rate]), rate))
        stdout.write(format_recovery_rows(sum_recovery_rows(tables[rate])))
    return 1 if failed else 0


def _supersample(args, stdin, stdout):
    """create_supersample.py for one id list or several: the sums on the GPU in one call, the files in one pass over
    --junction-file."""
    from .junctions import STORE_SUFFIX, JunctionStore, parse_groups_file, parse_sample_ids_file, write_supersample_files
    if args.sample_ids is not None:
        groups = [("supersample", parse_sample_ids_file(args.sample_ids))]
        paths = [args.output]
    else:
        groups = parse_groups_file(args.groups)
        paths = [args.output + "." + label for label, _ in groups]
    _require_store(args)
    store = JunctionStore.load(args.basename + STORE_SUFFIX, device=int(str(args.device).split(',')[0]))
    pooled = store.pool([ids for _, ids in groups])
    write_supersample_files(args.junction_file, zip(paths, pooled))
    for (label, ids), r in zip(groups, pooled):
        stdout.write("# group %s\tsamples %d\tjunctions %d\tcoverage %d\n"
                     % (label, len(set(ids)), len(r), sum(r.sums.tolist())))
    return 0


def _search_supersamples(args, searcher, stdout):
    """search --supersamples: every group pooled in one call and searched in one batch; a block per group, printed as
    --intropolis prints a sample's."""
    from .junctions import parse_groups_file
    groups = parse_groups_file(args.supersamples)
    if not groups:
        return 0
    labels = [label for label, _ in groups]
    pooled = searcher.pool_samples([ids for _, ids in groups])
    if args.unhashed:
        results = _unhashed_search(args, searcher, searcher.unhashed_terms_from_pooled(pooled, labels), args.results)
    else:
        results = _batch_search(args, searcher, searcher.queries_from_pooled(pooled, labels, args.unhashed_junction_file), args.results)
    return _write_blocks(stdout, labels, results, lambda label: stdout.write("# query %s\n" % label))


def _search_unhashed(args, searcher, stdin, stdout):
    """search --unhashed: the queries of `search`, ranked in the space of the junctions themselves; printed as `search`
    prints them."""
    from .junctions import intropolis_query_terms, key_lines, query_terms
    from .search import results_output
    by_item = args.query_ids if args.query_ids is not None else ([args.query_id] if args.query_id is not None else None)
    if by_item is not None:
        results = searcher.unhashed_search_member_n_batch(by_item, args.results, include_distances=args.distances,
                                                          meta_db=args.metadata, restriction=_restriction(args))
        for query_id, res in zip(by_item, results):
            _write_member_header(stdout, query_id, searcher.internal_id_map[query_id], args.query_ids is not None)
            results_output(res, stdout)
        return 0
    store, w = searcher.unhashed_store()
    key_line = key_lines(args.unhashed_junction_file, store.n_lines)
    if args.intropolis is not None:
        sample_ids, terms = intropolis_query_terms(args.intropolis, key_line, w)
        for sample_id, res in zip(sample_ids, _unhashed_search(args, searcher, terms, args.results)):
            stdout.write("# query %d\n" % sample_id)
            results_output(res, stdout)
        return 0
    coverage = _stream_coverage(_stream_parser(args.format)(stdin))
    results_output(_unhashed_search(args, searcher, [query_terms(coverage, key_line, w)], args.results)[0], stdout)
    return 0


def _search_radius_members(args, searcher, stdout, query_ids, numbered, collect=None):
    """-q / --query-ids under --max-distance: the header lines of the by-sample search, then every sample within the
    distance of the stored row, exactly (the query itself leads its list unless --leave-out-groups leaves it out)."""
    results = _batch_search(args, searcher, query_ids, None)
    return _write_blocks(stdout, query_ids, results,
                         lambda query_id: _write_member_header(stdout, query_id, searcher.internal_id_map[query_id], numbered), collect)


def _search_batch(args, searcher, stdout, collect=None):
    """--intropolis / --query-ids: one block per query, in query order; 1 when some exact query failed as the
    reference's would (math domain error), after all blocks.  collect: a list that receives (sample id, results) of
    every answered query."""
    from .search import results_output
    if args.query_ids is not None and _max_distance(args) is not None:
        return _search_radius_members(args, searcher, stdout, args.query_ids, True, collect)
    if args.query_ids is not None:
        internal, results = searcher.search_member_n_batch(args.query_ids, args.results, _search_k(args),
                                                           include_distances=args.distances, meta_db=args.metadata,
                                                           restriction=_restriction(args), n_trees=_use_trees(args))
        for query_id, internal_id, res in zip(args.query_ids, internal, results):
            _write_member_header(stdout, query_id, internal_id, True)
            results_output(res, stdout)
            if collect is not None:
                collect.append((query_id, res))
        return 0
    batch = searcher.queries_from_intropolis(args.intropolis)
    return _write_blocks(stdout, batch.ext_ids, _batch_search(args, searcher, batch, args.results),
                         lambda sample_id: stdout.write("# query %d\n" % sample_id), collect)


def _search(args, searcher, stdin, stdout, dist, rank, collect=None):
    """collect: a list that receives (label, results) of every query answered (`junctions` goes on from there)."""
    from .search import results_output
    if args.intropolis is not None or args.query_ids is not None:
        return _search_batch(args, searcher, stdout, collect)
    if args.query_id is not None and _max_distance(args) is not None:
        return _search_radius_members(args, searcher, stdout, [args.query_id], False, collect)
    if args.query_id is not None and _restriction(args) is not None:
        # search_member_n under a restriction: its two lines, then the restricted search by item
        internal, results = searcher.search_member_n_batch([args.query_id], args.results, _search_k(args),
                                                           include_distances=args.distances, meta_db=args.metadata,
                                                           restriction=_restriction(args))
        _write_member_header(stdout, args.query_id, internal[0], False)
        results_output(results[0], stdout)
        if collect is not None:
            collect.append((args.query_id, results[0]))
        return 0
    if args.query_id is not None:                              # morna.py:1358-1365
        if dist is not None and rank != 0:
            import contextlib
            with contextlib.redirect_stdout(stdout):           # ("querying by sample id ..." is rank 0's to print)
                results = searcher.search_member_n(args.query_id, args.results, args.search_k,
                                                   include_distances=args.distances, meta_db=args.metadata, n_trees=_use_trees(args))
        else:
            results = searcher.search_member_n(args.query_id, args.results, args.search_k,
                                               include_distances=args.distances, meta_db=args.metadata, n_trees=_use_trees(args))
        results_output(results, stdout)
        if collect is not None:
            collect.append((args.query_id, results))
        return 0
    if dist is not None:
        # only rank 0 has the stream: it parses it and every rank walks the same list of junctions
        box = [None]
        if rank == 0:
            box[0] = list(_stream_parser(args.format)(stdin))
        dist.broadcast_object_list(box, src=0)
        junction_generator = iter(box[0])
    else:
        junction_generator = _stream_parser(args.format)(stdin)
    if args.rawlist:
        for junction in junction_generator:
            stdout.write(str(junction) + "\n")
        return 0
    converge = bool(args.convergence_backoff) and args.format == 'sam'      # morna.py:1378
    backoff = args.convergence_backoff
    checkpoint = args.checkpoint
    old_results = [-1 for _ in range(args.results)]
    i = -1
    for i, junction in enumerate(junction_generator):          # morna.py:1383-1472
        string_junction = " ".join(str(_) for _ in junction[:3])
        if args.verbose and i % 1000 == 0:
            sys.stderr.write(str(i) + " junctions into query sample\r")
            sys.stderr.flush()
        if string_junction in searcher.sample_frequencies:
            searcher.update_query(junction)
        if converge and i == checkpoint:
            checkpoint += backoff
            backoff += backoff
            sys.stderr.write("\n")
            searcher.finalize_query()
            results = searcher.search_nn(args.results, args.search_k, include_distances=args.distances,
                                         meta_db=args.metadata, n_trees=_use_trees(args))
            same = True
            for j, result in enumerate(results[0]):
                if not (result == old_results[j]):
                    same = False
            if same:
                if args.verbose:
                    sys.stderr.write("Converged after " + str(i) + " junctions.\n")
                results_output(results, stdout)
                return 0
            if args.verbose:
                sys.stderr.write("Not converged after " + str(i) + " junctions.\n")
                sys.stderr.write("Old results:\n" + str(old_results) + "\n")
                sys.stderr.write("New results:\n" + str(results[0]) + "\n")
            old_results = results[0]
    if converge and args.verbose:
        sys.stderr.write("No convergence after " + str(i) + " junctions, but here's results:\n")
    searcher.finalize_query()
    if args.verbose:
        sys.stderr.write("\n")
    if _max_distance(args) is not None:
        results = searcher.exact_radius_nn(_max_distance(args), num_neighbors=_radius_cap(args), include_distances=args.distances,
                                           meta_db=args.metadata, restriction=_restriction(args))
    elif _restriction(args) is not None:
        if args.exact:
            results = searcher.exact_search_nn(args.results, include_distances=args.distances, meta_db=args.metadata,
                                               restriction=_restriction(args))
        else:
            results = searcher.search_nn(args.results, _search_k(args), include_distances=args.distances, meta_db=args.metadata,
                                         restriction=_restriction(args))
    elif args.exact and not converge:
        results = searcher.exact_search_nn(args.results, include_distances=args.distances, meta_db=args.metadata)
    else:
        results = searcher.search_nn(args.results, args.search_k, include_distances=args.distances,
                                     meta_db=args.metadata, n_trees=_use_trees(args))
    results_output(results, stdout)
    if collect is not None:
        collect.append((None, results))
    return 0


_THIN_POOL = (_check_downsample_flags, _check_supersample_flags)
# subcommand: (its flag checks in the order they run, its function of (args, stdin, stdout))
_COMMANDS = {
    'index': ((), _index),
    'search': (_THIN_POOL + (_check_batch_flags, _check_unhashed_flags, _check_restriction_flags, _check_use_trees_flags,
                             _check_max_distance_flags), _searching),
    'junctions': (_THIN_POOL + (_check_batch_flags, _check_unhashed_flags, _check_junction_flags, _check_restriction_flags),
                  _searching),
    'recovery': (_THIN_POOL + (_check_recovery_flags, _check_batch_flags, _check_restriction_flags), _searching),
    'supersample': ((), _supersample),
    'pairs': ((_check_pairs_flags,), _pairs),
    'recall': ((_check_recall_flags,), _recall),
    'hashing': ((_check_hashing_flags,), _hashing),
    'labels': ((_check_labels_flags,), _labels),
    'cluster': ((_check_cluster_flags,), _cluster),
    'mixture': ((_check_mixture_flags,), _mixture),
    'explain': ((_check_explain_flags,), _explain),
}


def main(argv=None, stdin=None, stdout=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if argv[:1] == ['pca']:                                    # (a parser of its own: build_parser() stays as it is pinned)
        parser = build_pca_parser()
        args = parser.parse_args(argv[1:])
        _check_pca_flags(parser, args)
        return _pca(args, stdin or sys.stdin, stdout or sys.stdout)
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.subparser_name is None:
        build_parser().print_help()
        return 2
    checks, command = _COMMANDS[args.subparser_name]
    for check in checks:
        check(parser, args)
    return command(args, stdin or sys.stdin, stdout or sys.stdout)


if __name__ == '__main__':
    sys.exit(main())
