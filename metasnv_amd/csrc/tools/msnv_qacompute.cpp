// msnv_qacompute -- process-level drop-in for `qaCompute [-c INT] [-q INT] [-m] [-p INT] [-x FILE] [-a SEED.FRAC] -d -i <in.bam> <out>`:
// metaSNV.py:63-65 invokes it with -c 10 -d -i (argv: src/qaTools/qaCompute.cpp:312-359; outputs OUT and OUT.detail,
// OUT.profile with -p and OUT.specific with -x :380-405; "Printing details in ..." on stdout :387; exit status 1 for
// usage / unopenable files :356-359,376-379, 0 on success :680).
// A thin main over the C ABI (include/msnv.h): all arithmetic runs on the GPU.  The options of qaCompute that are
// not built (-s -h) are rejected instead of being silently ignored.  -a SEED.FRAC (qaCompute.cpp:319-325: strtol, then strtod of what is
// left) subsamples the reads by the hash of their name on the GPU (msnv_coverage_sub); a fraction <= 0 ("-a 1") subsamples nothing.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <unistd.h>

#include "../../../include/msnv.h"

static void usage() {
    fprintf(stderr, "Usage: msnv_qacompute [-c INT] [-q INT] [-m] [-p INT] [-x FILE] [-a SEED.FRAC] -d [-i] <in.bam> <output.out>\n"
                    "  -c INT  maximum coverage of the breadth histogram (1..15, default 10 as metaSNV passes it)\n"
                    "  -q INT  minimum mapping quality (default 1)\n"
                    "  -d      write <output.out>.detail (always written; metaSNV.py always passes -d)\n"
                    "  -i      silent\n"
                    "  -m      add the Median_Cov column to <output.out>\n"
                    "  -p INT  write the coverage profile of windows of INT bases to <output.out>.profile (INT >= 1)\n"
                    "  -x FILE write the mean coverage of the regions in FILE (name start end alias) to <output.out>.specific\n"
                    "  -a SEED.FRAC  subsample the reads by the hash of their name: integer part = seed, fraction = share kept\n"
                    "          (42.25: seed 42, a quarter of the reads; mates stay together; a fraction of 0 keeps everything)\n"
                    "  -s INT, -h FILE of qaCompute are not supported\n");
}

int main(int argc, char **argv) {
    int max_cov = 10, min_mapq = 1, arg, median = 0, window = 0;
    bool profile = false, subsample = false;
    long long seed = 0; double frac = 0;
    const char *regions = nullptr;
    while ((arg = getopt(argc, argv, "mdip:s:q:c:h:x:a:")) >= 0) {
        switch (arg) {
        case 'd': case 'i': break;
        case 'q': min_mapq = atoi(optarg); break;
        case 'c': max_cov = atoi(optarg); break;
        case 'm': median = 1; break;
        case 'p': window = atoi(optarg); profile = true; break;
        case 'x': regions = optarg; break;
        case 'a': { char *q = nullptr; seed = strtoll(optarg, &q, 10); frac = strtod(q, &q); subsample = true; break; }
        default:
            fprintf(stderr, "msnv_qacompute: option -%c of qaCompute is not supported (metaSNV.py never passes it)\n", arg);
            return 1;
        }
    }
    if (argc - optind != 2 || (profile && window < 1)) { usage(); return 1; }
    const std::string out = argv[optind + 1], detail = out + ".detail", prof = out + ".profile", spec = out + ".specific";
    uint32_t word = 0;                                      // (a seed the rule refuses: before the device is asked for)
    if (subsample && msnv_subsample_seed_word(seed, &word)) { fprintf(stderr, "msnv_qacompute: -a: %s\n", msnv_last_error()); return 1; }
    msnv_ctx *ctx = nullptr;
    if (msnv_ctx_create(0, &ctx)) { fprintf(stderr, "msnv_qacompute: %s\n", msnv_last_error()); return 1; }
    fprintf(stdout, "Printing details in %s!\n", detail.c_str());
    int rc;
    if (subsample) {
        msnv_cov_ex_args a{};
        a.bam_path = argv[optind]; a.max_cov = max_cov; a.min_mapq = min_mapq;
        a.out_cov_path = out.c_str(); a.out_detail_path = detail.c_str();
        a.want_median = median; a.window = window; a.out_profile_path = prof.c_str();
        a.regions_path = regions; a.out_specific_path = spec.c_str();
        rc = msnv_coverage_sub(ctx, &a, word, frac);
    }
    else if (!median && !profile && !regions) {                 // the argv of metaSNV.py: the path it has always taken
        msnv_cov_args a{};
        a.bam_path = argv[optind]; a.max_cov = max_cov; a.min_mapq = min_mapq;
        a.out_cov_path = out.c_str(); a.out_detail_path = detail.c_str();
        rc = msnv_coverage(ctx, &a);
    }
    else {
        msnv_cov_ex_args a{};
        a.bam_path = argv[optind]; a.max_cov = max_cov; a.min_mapq = min_mapq;
        a.out_cov_path = out.c_str(); a.out_detail_path = detail.c_str();
        a.want_median = median; a.window = window; a.out_profile_path = prof.c_str();
        a.regions_path = regions; a.out_specific_path = spec.c_str();
        rc = msnv_coverage_ex(ctx, &a);
    }
    if (rc) fprintf(stderr, "msnv_qacompute: %s\n", msnv_last_error());
    msnv_ctx_destroy(ctx);
    return rc ? 1 : 0;
}
