// metasnv_amd/csrc/hclust.cpp -- host side of the row order of subpopr's report heatmaps (src/subpopr/inst/rmd/detailedSpeciesReport.rmd:142,
// :222, :250, :402: heatmap(hclustfun = hclust(method = ...)); the kernel and its launch are hclust_k.hip).
//
//   msnv_hclust_tasks    hclust of many (index list, method) tasks of one distance matrix: merge, height, order
//   msnv_heatmap_order   reorder(as.dendrogram(hc), weights) and order.dendrogram: host only
//   msnv_heatmap_file    the stage: the tree of every sample (average) and of the discovery subset (complete) in one call of the array form,
//                        rowMeans, the reorder, and the four files
// What is on the host: reading and writing, the checks, the cut of a batch into launches under the scratch budget, and O(m) bookkeeping per
// task -- the steps (a, b, h) the kernel leaves become merge and order; rowMeans and the reorder of the dendrogram.  Every distance update and
// every search for a minimum is on the device; there is no CPU fallback.
// Divergences: ties that a Lance-Williams update creates at a smaller column are taken, where R's lazily repaired
// nearest-neighbour list keeps the old column; the four files are ours, the reference keeps these numbers as pixels.
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "dataset.h"
#include "device.h"
#include "knobs.h"

namespace msnv {

namespace {

constexpr uint64_t HCLUST_MAX_ENTRIES = 1ull << 26;                    // list entries of one call

// The steps of one task to R's hc$merge (row by row) and hc$order (0-based)
void steps_to_tree(uint32_t m, const int32_t *a, const int32_t *b, int32_t *merge, int32_t *order) {
    std::vector<int32_t> label(m);
    for (uint32_t p = 0; p < m; ++p) label[p] = -(int32_t)(p + 1);
    for (uint32_t s = 1; s < m; ++s) {
        int32_t la = label[a[s - 1]], lb = label[b[s - 1]];
        if ((la > 0 && lb < 0) || (la > 0 && lb > 0 && lb < la)) std::swap(la, lb);    // a singleton first; of two clusters the smaller step
        merge[2 * (s - 1)] = la; merge[2 * (s - 1) + 1] = lb;
        label[a[s - 1]] = (int32_t)s;
    }
    std::vector<int32_t> stack{(int32_t)(m - 1)};                      // the leaves left to right, the first entry of a row to the left
    uint32_t out = 0;
    while (!stack.empty()) {
        const int32_t e = stack.back();
        stack.pop_back();
        if (e < 0) { order[out++] = -e - 1; continue; }
        stack.push_back(merge[2 * (e - 1) + 1]);
        stack.push_back(merge[2 * (e - 1)]);
    }
}

// is merge[m - 1][2] a tree in hc$merge's encoding: every singleton and every step but the last is a child exactly once, a step of an earlier row
bool merge_is_tree(uint32_t m, const int32_t *merge) {
    std::vector<uint8_t> leaf(m, 0), step(m, 0);
    for (uint32_t s = 1; s < m; ++s)
        for (int c = 0; c < 2; ++c) {
            const int64_t e = merge[2 * (s - 1) + c];
            if (e < 0) { if (-e > (int64_t)m || leaf[-e - 1]) return false; leaf[-e - 1] = 1; }
            else { if (e == 0 || e >= (int64_t)s || step[e]) return false; step[e] = 1; }
        }
    return true;                                                       // 2 (m - 1) distinct children of m + (m - 2) candidates: all are used
}

void reorder(uint32_t m, const int32_t *merge, const double *weights, int32_t *order) {
    std::vector<int32_t> kids(2 * (size_t)(m - 1));
    std::vector<double> value(m);                                      // of the node made at step s
    auto of = [&](int32_t e) { return e < 0 ? weights[-e - 1] : value[e]; };
    for (uint32_t s = 1; s < m; ++s) {
        int32_t l = merge[2 * (s - 1)], r = merge[2 * (s - 1) + 1];
        if (of(l) > of(r)) std::swap(l, r);
        kids[2 * (s - 1)] = l; kids[2 * (s - 1) + 1] = r;
        value[s] = (double)((long double)of(l) + (long double)of(r));
    }
    std::vector<int32_t> stack{(int32_t)(m - 1)};
    uint32_t out = 0;
    while (!stack.empty()) {
        const int32_t e = stack.back();
        stack.pop_back();
        if (e < 0) { order[out++] = -e - 1; continue; }
        stack.push_back(kids[2 * (e - 1) + 1]);
        stack.push_back(kids[2 * (e - 1)]);
    }
}

// Checked tasks on a resident matrix: launches under the scratch budget (a task above it is a launch of its own), then the trees
int run_tasks(msnv_ctx *ctx, const ClusterDev &dev, uint64_t n_tasks, const uint32_t *m, const uint32_t *method, const int32_t *idx, int32_t *merge, double *height,
              int32_t *order, double *ms_kernel) {
    uint64_t total = 0;
    for (uint64_t t = 0; t < n_tasks; ++t) total += m[t];
    std::vector<int32_t> a(total - n_tasks), b(total - n_tasks);
    const uint64_t budget = knob::hclust_scratch_bytes();
    uint64_t off0 = 0;
    for (uint64_t t0 = 0; t0 < n_tasks;) {
        uint64_t t1 = t0, bytes = 0, entries = 0;
        do { bytes += 8ull * m[t1] * m[t1]; entries += m[t1]; ++t1; } while (t1 < n_tasks && bytes + 8ull * m[t1] * m[t1] <= budget);
        if (int rc = dev_hclust_batch(dev, t1 - t0, m + t0, method + t0, idx + off0, ctx->stream, a.data() + (off0 - t0), b.data() + (off0 - t0), height + (off0 - t0), ms_kernel))
            return rc;
        off0 += entries; t0 = t1;
    }
    uint64_t off = 0;
    for (uint64_t t = 0; t < n_tasks; ++t) {
        steps_to_tree(m[t], a.data() + (off - t), b.data() + (off - t), merge + 2 * (off - t), order + off);
        off += m[t];
    }
    return MSNV_OK;
}

// rowMeans of the sub-matrix of `members`: a long double sum over ascending columns, divided by m
std::vector<double> row_means(const std::vector<double> &d, size_t n, const std::vector<int32_t> &members) {
    std::vector<double> w(members.size());
    for (size_t r = 0; r < members.size(); ++r) {
        long double sum = 0;
        for (int32_t c : members) sum += d[(size_t)members[r] * n + c];
        w[r] = (double)(sum / (long double)members.size());
    }
    return w;
}

}  // namespace
}  // namespace msnv

using namespace msnv;

extern "C" int msnv_hclust_tasks(msnv_ctx *ctx, int32_t n, const double *dist, int64_t n_tasks, const int32_t *task_m, const int32_t *task_method, const int32_t *idx,
                                 int32_t *merge, double *height, int32_t *order, double *ms_kernel) {
    clear_error();
    if (!ctx || !dist || !task_m || !task_method || !idx || !merge || !height || !order) return fail(MSNV_EINVAL, "msnv_hclust_tasks: NULL argument");
    if (n_tasks < 1) return fail(MSNV_EINVAL, "msnv_hclust_tasks: %lld tasks (at least 1)", (long long)n_tasks);
    if (ms_kernel) *ms_kernel = 0;
    if (int rc = check_matrix("msnv_hclust_tasks", n, dist)) return rc;
    std::vector<uint32_t> m((size_t)n_tasks), method((size_t)n_tasks);
    std::vector<int64_t> seen((size_t)n, -1);
    uint64_t off = 0;
    for (int64_t t = 0; t < n_tasks; ++t) {
        if (task_method[t] < MSNV_HCLUST_AVERAGE || task_method[t] > MSNV_HCLUST_MCQUITTY) return fail(MSNV_EINVAL, "msnv_hclust_tasks: task %lld has method %d", (long long)t, task_method[t]);
        if (task_m[t] < 2 || task_m[t] > n) return fail(MSNV_EDOMAIN, "msnv_hclust_tasks: task %lld has m = %d (2 <= m <= n = %d)", (long long)t, task_m[t], n);
        if (off + (uint64_t)task_m[t] > HCLUST_MAX_ENTRIES)
            return fail(MSNV_ECAPACITY, "msnv_hclust_tasks: more than %llu list entries in one call", (unsigned long long)HCLUST_MAX_ENTRIES);
        for (int32_t j = 0; j < task_m[t]; ++j) {
            const int32_t v = idx[off + j];
            if (v < 0 || v >= n) return fail(MSNV_EDOMAIN, "msnv_hclust_tasks: task %lld lists sample %d of %d", (long long)t, v, n);
            if (seen[v] == t) return fail(MSNV_EDOMAIN, "msnv_hclust_tasks: task %lld lists sample %d twice", (long long)t, v);
            seen[v] = t;
        }
        m[t] = (uint32_t)task_m[t]; method[t] = (uint32_t)task_method[t]; off += m[t];
    }
    if (int rc = dev_set_device(ctx->device)) return rc;
    ClusterDev dev;
    if (int rc = dev_cluster_upload(dev, dist, (uint32_t)n, ctx->stream)) return rc;
    return run_tasks(ctx, dev, (uint64_t)n_tasks, m.data(), method.data(), idx, merge, height, order, ms_kernel);
}

extern "C" int msnv_heatmap_order(int32_t m, const int32_t *merge, const double *weights, int32_t *order) {
    clear_error();
    if (!merge || !weights || !order) return fail(MSNV_EINVAL, "msnv_heatmap_order: NULL argument");
    if (m < 2) return fail(MSNV_EINVAL, "msnv_heatmap_order: %d leaves (at least 2)", m);
    if (!merge_is_tree((uint32_t)m, merge)) return fail(MSNV_EINVAL, "msnv_heatmap_order: merge is not the tree of %d leaves in hclust's encoding", m);
    for (int32_t p = 0; p < m; ++p)
        if (!std::isfinite(weights[p])) return fail(MSNV_EDOMAIN, "msnv_heatmap_order: the weight of leaf %d is %g", p, weights[p]);
    reorder((uint32_t)m, merge, weights, order);
    return MSNV_OK;
}

extern "C" int msnv_heatmap_file(msnv_ctx *ctx, const char *dist_path, const char *dir, const char *species, int64_t result[8], double *ms_kernel) {
    clear_error();
    if (!ctx || !dist_path || !dir || !species) return fail(MSNV_EINVAL, "msnv_heatmap_file: NULL argument");
    if (result) for (int i = 0; i < 8; ++i) result[i] = 0;
    if (ms_kernel) *ms_kernel = 0;
    std::vector<std::string> names;
    std::vector<double> d;
    if (int rc = read_dist(dist_path, names, d)) return rc;
    const size_t n = names.size();
    if (int rc = check_matrix(dist_path, (int64_t)n, d.data())) return rc;
    const std::string prefix = std::string(dir) + "/" + species + "_mann";

    // ---- the discovery subset: the names in the header of the matrix the medoids were defined on
    std::vector<std::vector<int32_t>> members(1);
    for (size_t i = 0; i < n; ++i) members[0].push_back((int32_t)i);
    const std::string used_path = prefix + "_distMatrixUsedForClustMedoidDefns.txt";
    if (file_exists(used_path)) {
        std::string text;
        if (int rc = slurp(used_path, text)) return rc;
        const char *s = text.data(), *e = (const char *)memchr(s, '\n', text.size());
        if (!e) e = s + text.size();
        if (e > s && e[-1] == '\r') --e;
        std::vector<Span> f;
        if (e > s) split_span(s, e, '\t', f);
        std::unordered_map<std::string, int32_t> at;
        for (size_t i = 0; i < n; ++i) at.emplace(names[i], (int32_t)i);
        std::vector<int32_t> sub;
        std::vector<uint8_t> listed(n, 0);
        for (const Span &c : f) {
            const std::string name(c.first, c.second);
            auto it = at.find(name);
            if (it == at.end()) return fail(MSNV_EFORMAT, "%s: sample '%s' is not in %s", used_path.c_str(), name.c_str(), dist_path);
            if (listed[it->second]) return fail(MSNV_EFORMAT, "%s: sample '%s' is listed twice", used_path.c_str(), name.c_str());
            listed[it->second] = 1;
            sub.push_back(it->second);
        }
        if (sub.size() >= 2) members.push_back(sub);
    }
    std::unordered_map<std::string, std::string> clust;
    const std::string clust_path = prefix + "_clustering.tab";
    const bool have_clust = file_exists(clust_path);
    if (have_clust) if (int rc = read_r_column(clust_path, "clust", clust)) return rc;
    if (int rc = dev_set_device(ctx->device)) return rc;

    // ---- both trees in one call of the array form
    const uint32_t n_trees = (uint32_t)members.size();
    std::vector<uint32_t> m, method;
    std::vector<int32_t> idx;
    for (uint32_t t = 0; t < n_trees; ++t) {
        m.push_back((uint32_t)members[t].size());
        method.push_back(t == 0 ? MSNV_HCLUST_AVERAGE : MSNV_HCLUST_COMPLETE);
        idx.insert(idx.end(), members[t].begin(), members[t].end());
    }
    std::vector<int32_t> merge(2 * (idx.size() - n_trees)), order(idx.size());
    std::vector<double> height(idx.size() - n_trees);
    ClusterDev dev;
    if (int rc = dev_cluster_upload(dev, d.data(), (uint32_t)n, ctx->stream)) return rc;
    if (int rc = run_tasks(ctx, dev, n_trees, m.data(), method.data(), idx.data(), merge.data(), height.data(), order.data(), ms_kernel)) return rc;

    // ---- the files
    std::vector<uint8_t> in_discovery(n, 0);
    if (n_trees > 1) for (int32_t i : members[1]) in_discovery[i] = 1;
    size_t off = 0;
    for (uint32_t t = 0; t < n_trees; ++t) {
        const uint32_t mt = m[t];
        const int32_t *mg = merge.data() + 2 * (off - t), *ord = order.data() + off;
        const double *h = height.data() + (off - t);
        const char *which = t == 0 ? "_all.tab" : "_discovery.tab";
        std::string text = "merge1\tmerge2\theight\n";
        for (uint32_t s = 1; s < mt; ++s) {
            text += std::to_string(s) + "\t" + std::to_string(mg[2 * (s - 1)]) + "\t" + std::to_string(mg[2 * (s - 1) + 1]) + "\t";
            r_value(h[s - 1], text);
            text.push_back('\n');
        }
        if (int rc = write_text(prefix + "_hclust" + which, text)) return rc;
        const std::vector<double> w = row_means(d, n, members[t]);
        std::vector<int32_t> heat(mt), pos(mt);
        reorder(mt, mg, w.data(), heat.data());
        for (uint32_t p = 0; p < mt; ++p) pos[ord[p]] = (int32_t)p;
        text = "index\thclustPos\tinDiscoverySubset\tclust\n";
        for (uint32_t r = 0; r < mt; ++r) {
            const int32_t p = heat[r], sample = members[t][p];
            auto it = clust.find(names[sample]);
            text += names[sample] + "\t" + std::to_string(p + 1) + "\t" + std::to_string(pos[p] + 1) + "\t" + (in_discovery[sample] ? "TRUE" : "FALSE") + "\t"
                    + (it == clust.end() ? std::string("NA") : it->second) + "\n";
        }
        if (int rc = write_text(prefix + "_heatmap" + which, text)) return rc;
        off += mt;
    }
    if (result) {
        result[0] = n_trees > 1 ? MSNV_HEATMAP_OK : MSNV_HEATMAP_NO_DISCOVERY;
        result[1] = (int64_t)n; result[2] = n_trees > 1 ? (int64_t)m[1] : 0; result[3] = have_clust ? 1 : 0;
    }
    return MSNV_OK;
}
