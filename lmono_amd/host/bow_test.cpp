// bow_test.cpp -- the loop detector's database on the host, without a GPU: the kernel bodies of ../csrc/bow.hip compiled as
// plain C++ (-ffp-contract=off) and driven by loops over (block, thread), piece by piece where the kernels have their barriers.
//   bow_test <case.bin> <results.bin>
// case: a vocabulary in the layout of VocabularyBinary.hpp (6 int32 k, L, scoringType, weightingType, nNodes, nWords; nNodes records
// int32 nodeId, int32 parentId, double weight, uint64 descriptor [4]; nWords records int32 nodeId, int32 wordId), then
//   int32 n_t, uint32 desc [n_t][8]                               descriptors to transform
//   int32 n_kf, int32 max_kp, per keyframe int32 n, uint32 desc [n][8]      the store
//   int32 n_q, per query int32 cur, max_results, max_id
//   int32 n_d, per detection int32 cur, loop_search_gap
// results: int32 refused; when refused int32 length and the message, nothing else.  Otherwise int32 word [n_t], double weight [n_t]; per
// keyframe int32 m, int32 word [m], double value [m]; per query int32 n, int32 id [n], double score [n]; per detection int32 loop index,
// int32 n, int32 id [n], double score [n].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/bow.hip"

using namespace lmono;

template <typename T> static bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <typename T> static bool wr(FILE *f, const T *p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

static int fail(const char *what) { fprintf(stderr, "bow_test: %s\n", what); return 1; }

static void run_words(const BowVoc &v, const BowWordsJob &j)
{
    const int blocks = (j.n + kBowT - 1) / kBowT;
    for (int b = 0; b < blocks; b++) for (int t = 0; t < kBowT; t++) bow_words_body(v, j, b, t);
}

static void run_vector(const BowVoc &v, BowVecJob j)
{
    if (j.n < 0) j.n = 0;
    const int P = bow_pow2(j.n);
    std::vector<int> lds((size_t)P), cnt((size_t)kBowT);
    for (int t = 0; t < kBowT; t++) bow_vec_load(v, j, P, lds.data(), t, kBowT);
    for (int k = 2; k <= P; k <<= 1)
        for (int jj = k >> 1; jj > 0; jj >>= 1)
            for (int t = 0; t < kBowT; t++) bow_vec_sort_step(lds.data(), P, k, jj, t, kBowT);
    for (int t = 0; t < kBowT; t++) cnt[(size_t)t] = bow_vec_count(lds.data(), P, t, kBowT);
    int m = 0;
    for (int t = 0; t < kBowT; t++) {
        int base = 0;
        for (int u = 0; u < t; u++) base += cnt[(size_t)u];
        bow_vec_emit(v, j, lds.data(), P, t, kBowT, base);
        m += cnt[(size_t)t];
    }
    if (m > j.n) m = j.n;
    const double norm = bow_vec_norm(j, m);
    *j.n_out = m;
    for (int t = 0; t < kBowT; t++) bow_vec_divide(j, m, norm, t, kBowT);
}

static void run_query(const BowQueryJob &j)
{
    const int blocks = (j.cur + kBowScoreT - 1) / kBowScoreT;
    for (int b = 0; b < blocks; b++) for (int t = 0; t < kBowScoreT; t++) bow_score_body(j, b, t, kBowScoreT);
    const int limit = bow_top_limit(j);
    bool have_last = false;
    double last_s = 0.0;
    int last_i = -1, n = 0;
    for (int r = 0; r < limit; r++) {
        std::vector<double> s((size_t)kBowT);
        std::vector<int> id((size_t)kBowT);
        for (int t = 0; t < kBowT; t++) bow_top_scan(j, t, kBowT, have_last, last_s, last_i, s[(size_t)t], id[(size_t)t]);
        for (int stride = kBowT / 2; stride > 0; stride >>= 1)
            for (int t = 0; t < stride; t++) bow_top_merge(s[(size_t)t], id[(size_t)t], s[(size_t)(t + stride)], id[(size_t)(t + stride)]);
        last_s = s[0]; last_i = id[0];
        if (last_i < 0) break;
        have_last = true;
        j.out->id[r] = last_i; j.out->score[r] = -last_s / 2.0;
        n++;
    }
    j.out->n = n; j.out->pad = 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: bow_test <case.bin> <results.bin>\n"); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "bow_test: cannot open the files\n"); return 2; }
    int32_t head[6];
    if (!rd(in, head, 6)) return fail("short header");
    const int32_t n_nodes = head[4], n_words = head[5];
    // the counts size the reads, so they are checked here already; bow_voc_build checks them again, with everything else
    const bool sane = n_nodes >= 0 && n_nodes <= 16777215 && n_words >= 0 && n_words <= 16777215;
    std::vector<int32_t> node_id, parent_id, word_node, word_id;
    std::vector<double> weight;
    std::vector<uint32_t> desc;
    if (sane) {
        const size_t n = (size_t)n_nodes, w = (size_t)n_words;
        node_id.resize(n); parent_id.resize(n); weight.resize(n); desc.resize(n * 8); word_node.resize(w); word_id.resize(w);
        for (size_t r = 0; r < n; r++)
            if (!rd(in, &node_id[r], 1) || !rd(in, &parent_id[r], 1) || !rd(in, &weight[r], 1) || !rd(in, &desc[r * 8], 8)) return fail("short node record");
        for (size_t r = 0; r < w; r++)
            if (!rd(in, &word_node[r], 1) || !rd(in, &word_id[r], 1)) return fail("short word record");
    }
    BowVocHost voc;
    // counts out of range: nothing was read, and bow_voc_build refuses them (or k, L, the types) before it looks at an array
    const char *why = sane ? bow_voc_build(head[0], head[1], head[2], head[3], n_nodes, node_id.data(), parent_id.data(), weight.data(), desc.data(), n_words,
                                           word_node.data(), word_id.data(), voc)
                           : bow_voc_build(head[0], head[1], head[2], head[3], n_nodes, nullptr, nullptr, nullptr, nullptr, n_words, nullptr, nullptr, voc);
    if (why) {
        const int32_t one = 1, len = (int32_t)strlen(why);
        if (!wr(out, &one, 1) || !wr(out, &len, 1) || !wr(out, why, (size_t)len)) return fail("write failed");
        fclose(in);
        return fclose(out) == 0 ? 0 : 1;
    }
    const int32_t zero = 0;
    if (!wr(out, &zero, 1)) return fail("write failed");
    const BowVoc v = voc.view();

    int32_t n_t = 0;
    if (!rd(in, &n_t, 1) || n_t < 0 || n_t > (1 << 24)) return fail("bad transform count");
    {
        std::vector<uint32_t> d((size_t)n_t * 8);
        std::vector<int> word((size_t)n_t, -2);
        std::vector<double> wt((size_t)n_t, -1.0);
        if (!rd(in, d.data(), d.size())) return fail("short transform descriptors");
        run_words(v, BowWordsJob{ d.data(), n_t, word.data(), wt.data() });
        if (!wr(out, word.data(), word.size()) || !wr(out, wt.data(), wt.size())) return fail("write failed");
    }

    int32_t n_kf = 0, max_kp = 0;
    if (!rd(in, &n_kf, 1) || !rd(in, &max_kp, 1) || n_kf < 0 || n_kf > 65535 || max_kp < 1 || max_kp > kBowMaxKp) return fail("bad store limits (max_keypoints 1..16384)");
    const size_t per = (size_t)max_kp;
    std::vector<int> bow_word((size_t)n_kf * per, -1), bow_n((size_t)n_kf, 0);
    std::vector<double> bow_val((size_t)n_kf * per, 0.0);
    for (int32_t f = 0; f < n_kf; f++) {
        int32_t n = 0;
        if (!rd(in, &n, 1) || n < 0 || n > max_kp) return fail("a keyframe with more descriptors than max_kp");
        std::vector<uint32_t> d((size_t)n * 8);
        if (!rd(in, d.data(), d.size())) return fail("short keyframe");
        int *row_w = bow_word.data() + (size_t)f * per;
        double *row_v = bow_val.data() + (size_t)f * per;
        run_words(v, BowWordsJob{ d.data(), n, row_w, nullptr });
        run_vector(v, BowVecJob{ n, row_w, row_v, &bow_n[(size_t)f] });
        const int32_t m = bow_n[(size_t)f];
        if (!wr(out, &m, 1) || !wr(out, row_w, (size_t)m) || !wr(out, row_v, (size_t)m)) return fail("write failed");
    }

    std::vector<double> s((size_t)n_kf + 1);
    std::vector<int> flag((size_t)n_kf + 1);
    BowResult res;
    BowQueryJob q{ bow_word.data(), bow_val.data(), bow_n.data(), max_kp, n_kf, 0, -1, 4, s.data(), flag.data(), &res };
    int32_t n_q = 0;
    if (!rd(in, &n_q, 1) || n_q < 0) return fail("bad query count");
    for (int32_t i = 0; i < n_q; i++) {
        int32_t a[3];
        if (!rd(in, a, 3) || a[0] < 0 || a[0] >= n_kf || a[1] < 1 || a[1] > kBowMaxResults) return fail("bad query (cur inside the store, max_results 1..16)");
        q.cur = a[0]; q.max_results = a[1]; q.max_id = a[2];
        run_query(q);
        const int32_t n = res.n;
        if (!wr(out, &n, 1) || !wr(out, res.id, (size_t)n) || !wr(out, res.score, (size_t)n)) return fail("write failed");
    }
    int32_t n_d = 0;
    if (!rd(in, &n_d, 1) || n_d < 0) return fail("bad detection count");
    for (int32_t i = 0; i < n_d; i++) {
        int32_t a[2];
        if (!rd(in, a, 2) || a[0] < 0 || a[0] >= n_kf) return fail("bad detection (cur inside the store)");
        q.cur = a[0]; q.max_results = 4; q.max_id = a[0] - a[1];
        run_query(q);
        const int32_t n = res.n, loop = bow_detect_rule(a[0], a[1], n, res.id, res.score);
        if (!wr(out, &loop, 1) || !wr(out, &n, 1) || !wr(out, res.id, (size_t)n) || !wr(out, res.score, (size_t)n)) return fail("write failed");
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
