"""metaSNV_DistDiv.py-compatible driver (reference: /metaSNV_DistDiv.py:105-139, 182-384): the pairwise distances
(`--dist`, msnv_dist_file) and the nucleotide diversity / FST (`--div`) and piN / piS (`--divNS`, msnv_div_file) computed
on the GPU, one call per species table.

Same argv and the same files: `--filt <proj>/filtered<pars>/pop` -> `<proj>/distances<pars>/` (`.matched_pos/` with
`--matched`): `<species>.filtered.mann.dist` / `.allele.dist`, `<species>.diversity` / `.FST`, `<species>.N_diversity` /
`.S_diversity`.  This module reads the coverage tables and bed_header and computes the row order sort_index applies
(numpy's argsort of the position keys); the library does the rest.  `--n_threads` is accepted and ignored."""
import argparse
import ctypes as C
import glob
import os
import sys
from datetime import datetime


def build_parser():                                            # metaSNV_DistDiv.py:31-57
    p = argparse.ArgumentParser(prog='metaSNV_DistDiv.py', description='metaSNV distances and diversity computation',
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--version', action='version', version='%(prog)s 2.0', help=argparse.SUPPRESS)
    p.add_argument("--debug", action="store_true", help=argparse.SUPPRESS)
    p.add_argument('--filt', metavar=': Filtered frequency files', help="Folder containing /pop/*.filtered.freq", required=True)
    p.add_argument('--dist', action='store_true', help="Compute distances")
    p.add_argument('--div', action='store_true', help="Compute Diversity and FST")
    p.add_argument('--divNS', action='store_true', help="Computing piN and piS")
    p.add_argument('--matched', action='store_true', help="Computing on matched positions only")
    p.add_argument('--n_threads', metavar=': Number of Processes', default=1, type=int, help="Number of jobs to run simultaneously (accepted, not used: the device runs every pair at once).")
    return p


def file_check(args):                                          # metaSNV_DistDiv.py:62-78 (same messages, same exit)
    parts = args.filt.rstrip('/').split('/')
    args.projdir = '/'.join(parts[:-2])                        # .../<proj>/filtered<pars>/pop -> <proj>
    args.pars = parts[-2].strip('filtered')
    stem = args.projdir + '/' + args.projdir.split('/')[-1]
    args.coverage_file, args.percentage_file = stem + '.all_cov.tab', stem + '.all_perc.tab'
    args.bedfile = args.projdir + '/' + 'bed_header'
    needed = (args.coverage_file, args.percentage_file, args.bedfile)
    print("Checking for necessary input files...")
    if not all(os.path.isfile(n) for n in needed):
        sys.exit("\nERROR: No such file '{}',\nERROR: No such file '{}',\nERROR: No such file '{}'".format(*needed))
    print("found: '{}' \nfound:'{}' \nfound:'{}'".format(*needed))


def compute_dist(ctx, filt_file, outdir, threshold=.6):        # metaSNV_DistDiv.py:113-124
    from ._lib import lib, check
    species = filt_file.split('/')[-1].replace('.freq', '')
    ns, npos, ms = C.c_int32(), C.c_uint64(), C.c_double()
    check(lib.msnv_dist_file(ctx._h, filt_file.encode(), (outdir + '/' + '%s.mann.dist' % species).encode(),
                             (outdir + '/' + '%s.allele.dist' % species).encode(), threshold, C.byref(ns), C.byref(npos), C.byref(ms)))
    return ns.value, npos.value, ms.value


class InputError(Exception):
    """A species or sample the coverage tables or bed_header do not hold (the reference raises KeyError there)."""


def read_tab(path):                                            # pd.read_table(path, skiprows=[1], index_col=0)
    """{species: {sample: value}} of <proj>.all_perc.tab / .all_cov.tab, the numbers read with pandas' converter.
    Species are looked up by their text (the reference's int index for all-numeric names fails: DESIGN.md section 7)."""
    from ._lib import lib, check
    with open(path) as f:
        lines = [l.rstrip('\r\n') for l in f]
    names = lines[0].split('\t')[1:] if lines else []
    tab = {}
    for lineno, line in enumerate(lines[2:], 3):
        if not line:
            continue
        fields = line.split('\t')
        row = {}
        for name, text in zip(names, fields[1:]):
            if text in ('', 'nan', 'NaN', 'NA', 'N/A', 'null', 'NULL', 'None', '<NA>'):
                row[name] = float('nan')
                continue
            v = C.c_double()
            if lib.msnv_parse_float(text.encode(), C.byref(v)) != 0:
                raise InputError("{}:{}: '{}' is not a number".format(path, lineno, text))
            row[name] = v.value
        tab[fields[0]] = row
    return tab


def genome_lengths(bedfile):                                   # metaSNV_DistDiv.py:316-318, 206
    """{species: L}: column 3 of bed_header summed over the contigs whose name, split at the first '.', is the species."""
    out = {}
    with open(bedfile) as f:
        for lineno, line in enumerate(f, 1):
            fields = line.rstrip('\r\n').split('\t')
            if fields == ['']:
                continue
            try:
                n = int(fields[2])
            except (IndexError, ValueError):
                raise InputError("{}:{}: no integer length in column 3".format(bedfile, lineno))
            sp = fields[0].split('.')[0]
            out[sp] = out.get(sp, 0) + n
    return out


def row_order(freq_path, stable):
    """The permutation DataFrame.sort_index applies to the table's contig:gene:pos keys: none when they are already
    monotonic, else numpy's argsort of the object array -- quicksort for --div (a plain Index: NOT stable, the order of
    tied rows feeds the arithmetic), stable for --divNS (the (key, N/S) MultiIndex is lexsorted)."""
    import numpy as np
    keys = []
    with open(freq_path) as f:
        next(f, None)
        for line in f:
            line = line.rstrip('\r\n')
            if line:
                keys.append(':'.join(line.split('\t', 1)[0].split(':')[:3]))
    k = np.array(keys, dtype=object)
    if len(k) < 2 or bool(np.all(k[:-1] <= k[1:])):
        return np.arange(len(k), dtype=np.int64)
    return k.argsort(kind='stable' if stable else 'quicksort').astype(np.int64)


def compute_div(ctx, filt_file, mode, matched, tabs, outdir):  # computeDiv / computeDivNS, metaSNV_DistDiv.py:182-301
    import numpy as np
    from ._lib import lib, check, DIV
    perc, cov, lengths = tabs
    species = filt_file.split('/')[-1].split('.')[0]
    with open(filt_file) as f:
        samples = f.readline().rstrip('\r\n').split('\t')[1:]
    for what, tab in (("the percentage table", perc), ("the coverage table", cov)):
        if species not in tab:
            raise InputError("species '{}' is not in {}".format(species, what))
        missing = [s for s in samples if s not in tab[species]]
        if missing:
            raise InputError("sample(s) {} of species '{}' are not in {}".format(', '.join(missing), species, what))
    if species not in lengths:
        raise InputError("species '{}' has no contig in bed_header".format(species))
    h = np.array([perc[species][s] for s in samples], dtype=np.float64)
    v = np.array([cov[species][s] for s in samples], dtype=np.float64)
    order = row_order(filt_file, stable=mode != DIV)
    names = ('%s.diversity', '%s.FST') if mode == DIV else ('%s.N_diversity', '%s.S_diversity')
    P = C.POINTER
    ns, nrows, ms = C.c_int32(), C.c_uint64(), C.c_double()
    check(lib.msnv_div_file(ctx._h, filt_file.encode(), mode, int(bool(matched)), lengths[species],
                            h.ctypes.data_as(P(C.c_double)), v.ctypes.data_as(P(C.c_double)), len(samples),
                            order.ctypes.data_as(P(C.c_int64)), len(order), (outdir + '/' + names[0] % species).encode(),
                            (outdir + '/' + names[1] % species).encode(), C.byref(ns), C.byref(nrows), C.byref(ms)))
    return ns.value, nrows.value, ms.value


def compute_all_div(ctx, args, outdir):                        # computeAllDiv, metaSNV_DistDiv.py:306-344
    from ._lib import DIV, DIV_NS
    print("Computing diversities & FST")
    tabs = (read_tab(args.percentage_file), read_tab(args.coverage_file), genome_lengths(args.bedfile))
    all_freq = glob.glob(args.filt + '/*.freq')
    for mode, wanted in ((DIV, args.div), (DIV_NS, args.divNS)):
        if wanted:
            for f in all_freq:
                compute_div(ctx, f, mode, args.matched, tabs, outdir)


def main(argv=None):                                           # metaSNV_DistDiv.py:355-384
    args = build_parser().parse_args(argv)
    file_check(args)
    outdir = args.projdir + '/distances' + args.pars + ('.matched_pos/' if args.matched else '/')
    if not os.path.exists(outdir):
        os.makedirs(outdir)
    print("Starting computations: ", datetime.now())
    if args.dist or args.div or args.divNS:
        from . import core
        try:
            ctx = core.Context(0)
        except core._lib.MsnvError as e:
            div = [o for o, on in (("--div", args.div), ("--divNS", args.divNS)) if on]
            sys.exit("\nERROR:  {}\n\nSOLUTION: run on a node with an AMD Instinct GPU ({}there is no CPU fallback)\n".format(
                e, "a CPU route for {} is not built; ".format(" / ".join(div)) if div else ""))
        try:
            if args.dist:
                print("Computing distances")
                for f in glob.glob(args.filt + '/*.freq'):
                    compute_dist(ctx, f, outdir)
            if args.div or args.divNS:
                compute_all_div(ctx, args, outdir)
        except (core._lib.MsnvError, InputError) as e:
            sys.exit("ERROR: {}".format(e))
        finally:
            ctx.close()
    print("Computations complete: ", datetime.now())


if __name__ == '__main__':
    main()
