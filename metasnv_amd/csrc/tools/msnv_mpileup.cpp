// msnv_mpileup -- process-level replacement of the left half of the pipe metaSNV.py:160-176 runs:
//   samtools mpileup -f REF [-l SPLIT] -B -b LIST [-q INT] [-Q INT] [-A] [-x] [-d INT] [--ff INT]  > pileup text
// and three options the driver does not pass: -a / -aa (a line for every position), -s (a MAPQ column), -O / --output-BP (a read-offset column).
// Same options, the text on stdout (or -o FILE) like samtools; the lines are formatted on the GPU (msnv_mpileup_text_ex).
//   msnv_mpileup -f REF -B -b LIST | snpCall -f REF -i INDIV -c C -t T > CALLED        runs the reference's caller on this pileup
// -B is REQUIRED: without it samtools recomputes the base qualities (BAQ), which is not built.  Every other samtools option is
// refused with exit status 1, never ignored.  Exit status: 0 ok, > 0 failure (the driver treats v > 0 as fatal, metaSNV.py:212-221).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <getopt.h>
#include <string>
#include <vector>

#include "../../../include/msnv.h"

static void usage() {
    fprintf(stderr, "Usage: msnv_mpileup -f REF.fa [-l BED] -B -b BAM_LIST [-q MIN_MAPQ=0] [-Q MIN_BASEQ=13] [-A] [-x] [-d MAX_DEPTH=8000]\n"
                    "                    [--ff FLAGS=0x704] [-a | -aa] [-s] [-O | --output-BP] [-o FILE] [-@ HOST_THREADS] > mpileup text\n"
                    "       -a: a line for every position of every contig that has reads, -aa (or -a -a): of every contig of the header\n"
                    "       -s: a mapping-quality column behind the qualities (spelled -s only; the long form --output-MQ is not taken)\n"
                    "       -O, --output-BP: a column of 1-based offsets in the read behind that\n"
                    "       -B is required (no BAQ: base qualities are never recomputed); other samtools options are not supported\n");
}

static bool parse_int(const char *s, int base, int *out) {
    char *end = nullptr;
    const long v = strtol(s, &end, base);
    if (end == s || *end) return false;
    *out = (int)v;
    return true;
}

int main(int argc, char **argv) {
    std::string ref, list, bed, out;
    msnv_params p;
    msnv_params_default(&p);
    msnv_mpileup_text_opts o;
    msnv_mpileup_text_opts_default(&o);
    int threads = 0, arg, no_baq = 0;
    static const option longopts[] = {{"ff", required_argument, nullptr, 1}, {"excl-flags", required_argument, nullptr, 1}, {"output-BP", no_argument, nullptr, 'O'},
                                      {nullptr, 0, nullptr, 0}};
    opterr = 0;
    while ((arg = getopt_long(argc, argv, "+f:l:b:q:Q:d:o:@:BAxasO", longopts, nullptr)) >= 0) {
        bool ok = true;
        switch (arg) {
        case 'f': ref = optarg; break;
        case 'l': bed = optarg; break;
        case 'b': list = optarg; break;
        case 'o': out = optarg; break;
        case 'B': no_baq = 1; break;
        case 'A': p.count_orphans = 1; break;
        case 'x': p.ignore_overlaps = 1; break;
        case 'a': if (o.all_positions < 2) ++o.all_positions; break;
        case 's': o.output_mq = 1; break;
        case 'O': o.output_bp = 1; break;
        case 'q': ok = parse_int(optarg, 10, &p.min_mapq); break;
        case 'Q': ok = parse_int(optarg, 10, &p.min_baseq); break;
        case 'd': ok = parse_int(optarg, 10, &p.max_depth); break;
        case '@': ok = parse_int(optarg, 10, &threads); break;
        case 1:   ok = parse_int(optarg, 0, &p.flag_filter); break;      // (decimal, 0x hex or 0 octal, like samtools)
        default:
            fprintf(stderr, "msnv_mpileup: option %s is not supported\n", optind > 0 && optind <= argc ? argv[optind - 1] : "?");
            usage();
            return 1;
        }
        if (!ok) { fprintf(stderr, "msnv_mpileup: %s is not a number\n", optarg); usage(); return 1; }
    }
    if (optind != argc) { fprintf(stderr, "msnv_mpileup: the BAM files come as a list (-b); %s is not an option\n", argv[optind]); usage(); return 1; }
    if (argc == 1 || list.empty() || ref.empty()) { usage(); return 1; }
    if (!no_baq) { fprintf(stderr, "msnv_mpileup: -B is required (BAQ is not built: without -B samtools recomputes the base qualities)\n"); return 1; }
    std::vector<std::string> bams;
    {
        std::ifstream in(list);
        if (!in) { fprintf(stderr, "msnv_mpileup: cannot open %s\n", list.c_str()); return 1; }
        for (std::string l; std::getline(in, l);) { while (!l.empty() && (l.back() == '\r' || l.back() == ' ')) l.pop_back(); if (!l.empty()) bams.push_back(l); }
    }
    if (bams.empty()) { fprintf(stderr, "msnv_mpileup: %s lists no BAM files\n", list.c_str()); return 1; }
    std::vector<const char *> paths;
    for (const std::string &b : bams) paths.push_back(b.c_str());
    msnv_ctx *ctx = nullptr;
    if (msnv_ctx_create(0, &ctx)) { fprintf(stderr, "msnv_mpileup: %s\n", msnv_last_error()); return 1; }
    msnv_mpileup_text_args a{};
    a.bam_paths = paths.data(); a.n_bams = (int32_t)paths.size();
    a.ref_fasta = ref.c_str();
    a.bed_split_path = bed.empty() ? nullptr : bed.c_str();
    a.out_path = out.empty() ? nullptr : out.c_str();
    a.host_threads = threads;
    a.params = p;
    const int rc = msnv_mpileup_text_ex(ctx, &a, &o, nullptr);
    if (rc) fprintf(stderr, "msnv_mpileup: %s\n", msnv_last_error());
    msnv_ctx_destroy(ctx);
    return rc;
}
