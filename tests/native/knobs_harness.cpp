// tests/native/knobs_harness.cpp -- one accessor of metasnv_amd/csrc/knobs.h, by name (tests/test_knobs.py; built with g++ from that
// header alone).  "knobs_harness ACCESSOR" prints what the accessor returns in the environment it was started with; with two more
// arguments, "ACCESSOR VAR VALUE", it then sets VAR=VALUE in its own environment and prints a second call on a second line: a per-call
// knob shows the new value there, a once-per-process knob the first one again.  Arguments that the library passes from other headers'
// constants (NARROW_MAX_DEPTH, GATE_MAX_TILES, ...) are plain numbers here, named in the table below.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../metasnv_amd/csrc/knobs.h"

using namespace msnv;

static std::string num(long long v) { return std::to_string(v); }
static std::string unum(unsigned long long v) { return std::to_string(v); }
static std::string chr(char c) { return c ? std::string(1, c) : std::string("-"); }      // "-": no choice made

struct Row { const char *name; std::string (*call)(); };
static const Row rows[] = {
    // first character
    {"pack_on_host", [] { return num(knob::pack_on_host()); }},
    {"lean_off", [] { return num(knob::lean_off()); }},
    {"item_taper", [] { return num(knob::item_taper()); }},
    {"merge_always", [] { return num(knob::merge_always()); }},
    {"guard_alloc", [] { return num(knob::guard_alloc()); }},
    {"depth_on_main", [] { return num(knob::depth_on_main()); }},
    {"finalize_trace", [] { return num(knob::finalize_trace()); }},
    {"crc_table", [] { return num(knob::crc_table()); }},
    {"merged_gather", [] { return num(knob::merged_gather()); }},
    // a choice, or none
    {"layout", [] { return chr(knob::layout()); }},
    {"fuse", [] { return chr(knob::fuse()); }},
    {"cov_index", [] { return chr(knob::cov_index()); }},
    {"stage_free", [] { return chr(knob::stage_free()); }},
    {"alleles", [] { return chr(knob::alleles()); }},
    {"inflate_where", [] { return chr(knob::inflate_where()); }},
    {"inflate_zlib", [] { return num(knob::inflate_zlib()); }},
    // present or absent
    {"cov_late", [] { return num(knob::cov_late()); }},
    {"no_adopt", [] { return num(knob::no_adopt()); }},
    {"debug_sync", [] { return num(knob::debug_sync()); }},
    // integers
    {"inflate_check_every", [] { return unum(knob::inflate_check_every()); }},
    {"inflate_batch_bytes", [] { return unum(knob::inflate_batch_bytes()); }},
    {"inflate_batch_bytes_resident", [] { return unum(knob::inflate_batch_bytes(true)); }},
    {"split_at_255", [] { return unum(knob::split_at(255)); }},
    {"group_depth", [] { return unum(knob::group_depth()); }},
    {"shallow_pieces", [] { return unum(knob::shallow_pieces()); }},
    {"fuse_pieces", [] { return unum(knob::fuse_pieces()); }},
    {"item_pieces", [] { return unum(knob::item_pieces()); }},
    {"tot_mode_min", [] { return unum(knob::tot_mode_min()); }},
    {"cov_item_intervals", [] { return unum(knob::cov_item_intervals()); }},
    {"cov_narrow_max", [] { return unum(knob::cov_narrow_max()); }},
    {"scan_sub_bytes_streams", [] { return unum(knob::scan_sub_bytes(knob::SCAN_SUB_STREAMS)); }},
    {"scan_sub_bytes_round", [] { return unum(knob::scan_sub_bytes(knob::SCAN_SUB_ROUND)); }},
    {"scan_seg_bytes", [] { return unum(knob::scan_seg_bytes()); }},
    {"pack_round_bytes", [] { return unum(knob::pack_round_bytes()); }},
    {"huge_pages", [] { return num(knob::huge_pages()); }},
    {"tail_skip", [] { return unum(knob::tail_skip()); }},
    {"dev_cache_mb", [] { return num(knob::dev_cache_mb()); }},
    {"text_repeat", [] { return num(knob::text_repeat()); }},
    {"stage_slab_rows", [] { return unum(knob::stage_slab_rows()); }},
    // integers over a default of the call site
    {"gather_split_2", [] { return unum(knob::gather_split(2)); }},
    {"chunk_cap_777", [] { return unum(knob::chunk_cap(777)); }},
    {"cap_events_1000_min_64", [] { return unum(knob::cap_events(1000, 64)); }},
    {"gate_tiles_4_max_8", [] { return unum(knob::gate_tiles(4, 8)); }},
    {"scatter_blocks_16", [] { return unum(knob::scatter_blocks(16)); }},
    {"text_chunk_bytes_4096", [] { return unum(knob::text_chunk_bytes(4096)); }},
    // the rest
    {"guard_fill", [] { int b = -1; return knob::guard_fill(&b) ? num(b) : std::string("-"); }},
    {"taper_at", [] { const knob::TaperAt t = knob::taper_at(); char s[96]; snprintf(s, sizeof s, "%g,%g,%g", t.u1, t.u2, t.u3); return std::string(s); }},
};

int main(int argc, char **argv) {
    if (argc != 2 && argc != 4) { fprintf(stderr, "usage: knobs_harness ACCESSOR [VAR VALUE]\n"); return 2; }
    for (const Row &r : rows) {
        if (strcmp(r.name, argv[1]) != 0) continue;
        puts(r.call().c_str());
        if (argc == 4) { setenv(argv[2], argv[3], 1); puts(r.call().c_str()); }
        return 0;
    }
    fprintf(stderr, "knobs_harness: no accessor %s\n", argv[1]);
    return 2;
}
