// loop_host_check -- the loop detectors' batch contract (csrc/loop_host.hpp)
// against an independent restatement of its rules, and the result record
// against one built by hand, on the host alone and under the sanitizers.
//
// check_loop_batch: batches of 0 to 3 queries with 0 to 3 candidates each,
// every first_candidate and num_candidates off by -1, 0 and +1, the declared
// number of candidates one less than, equal to and one more than the sum,
// every map and every scan null or not, and seven thresholds.  The full
// product of these has about 4e8 cases; the structure (counts, perturbations,
// declared total: 143 967 cases) is enumerated in full, and pointers and
// thresholds multiply in where they can decide the outcome or the product
// stays small (see cases_of()).
// Maps and scans are opaque: addresses of local dummies, never dereferenced.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "loop_host.hpp"

namespace {

int g_failed = 0;
long long g_cases = 0, g_accepted = 0;

void fail(const char* what, long long id)
{
    if (++g_failed <= 20) std::printf("FAIL %s (case %lld)\n", what, id);
}

struct Batch {
    std::vector<lgs_loop_query> qs;
    std::vector<lgs_loop_candidate> cs;   // exactly max(declared, 0) entries: an over-read is an ASan report
    int declared = 0;
};

// The rule, restated without the walk's running bound: thresholds in (0, 1];
// no null pointer; counts >= 0, the first range starts at 0, every range
// starts where the one before ends, and the last ends at the declared total.
bool oracle(double thr, const Batch& b, std::vector<int>& query_of)
{
    if (!(thr > 0 && thr <= 1)) return false;
    for (const auto& q : b.qs)
        if (!q.map) return false;
    for (const auto& c : b.cs)
        if (!c.scan) return false;
    long long end = 0;
    for (const auto& q : b.qs) {
        if (q.num_candidates < 0 || (long long)q.first_candidate != end) return false;
        end = (long long)q.first_candidate + q.num_candidates;
    }
    if (end != b.declared) return false;
    query_of.assign((size_t)b.declared, -1);
    for (int i = 0; i < b.declared; ++i)
        for (size_t q = 0; q < b.qs.size(); ++q)
            if (i >= b.qs[q].first_candidate && i < b.qs[q].first_candidate + b.qs[q].num_candidates) {
                if (query_of[(size_t)i] != -1) return false;   // covered twice: not a tiling
                query_of[(size_t)i] = (int)q;
            }
    for (int q : query_of)
        if (q < 0) return false;
    return true;
}

void one_case(double thr, const Batch& b)
{
    const long long id = g_cases++;
    std::vector<int> want, got;
    const bool ok = oracle(thr, b, want);
    bool accepted = true;
    int code = 0;
    try {
        got = lgs::check_loop_batch(thr, b.qs.empty() ? nullptr : b.qs.data(), (int)b.qs.size(),
                                    b.cs.empty() ? nullptr : b.cs.data(), b.declared, ":0-0");
    } catch (const lgs::Error& e) {
        accepted = false;
        code = e.code;
    }
    if (accepted != ok) return fail(ok ? "rejected a valid batch" : "accepted an invalid batch", id);
    if (!accepted && code != LGS_ERR_INVALID_ARG) return fail("status is not LGS_ERR_INVALID_ARG", id);
    if (accepted && got != want) return fail("query_of differs", id);
    g_accepted += accepted;
}

// The (map mask, scan mask, threshold) combinations tried on one structure.
// Thresholds run with valid pointers: all seven, but 0.5 alone on three
// queries whose structure is rejected anyway.  Pointers are nulled at
// threshold 0.5, every subset of maps with these subsets of scans: all of
// them up to one query, and on an accepted structure of up to four
// candidates; else, on two queries and on every accepted structure: none,
// each single scan and all scans.  Three queries, rejected structure: no
// pointer is nulled (each rejection costs a throw, about 5 us under the
// sanitizers, and there are 139 968 such structures).
void cases_of(Batch& b)
{
    static int map_dummy, scan_dummy;
    const double thresholds[] = { 0.0, -0.1, DBL_MIN, 0.5, 1.0, std::nextafter(1.0, 2.0), std::nan("") };
    const size_t nq = b.qs.size(), nc = b.cs.size();
    auto point = [&](unsigned maps_null, unsigned scans_null) {
        for (size_t q = 0; q < nq; ++q)
            b.qs[q].map = (maps_null >> q & 1) ? nullptr : (const lgs_grid*)&map_dummy;
        for (size_t c = 0; c < nc; ++c)
            b.cs[c].scan = (scans_null >> c & 1) ? nullptr : (const lgs_scan*)&scan_dummy;
    };
    point(0, 0);
    std::vector<int> unused;
    const bool structure_ok = oracle(0.5, b, unused);
    if (nq <= 2 || structure_ok)
        for (double thr : thresholds) one_case(thr, b);
    else
        one_case(0.5, b);
    const unsigned all_maps = (1u << nq) - 1, all_scans = (1u << nc) - 1;
    std::vector<unsigned> scans;
    if (nq <= 1 || (structure_ok && nc <= 4)) {
        for (unsigned s = 0; s <= all_scans; ++s) scans.push_back(s);
    } else if (nq == 2 || structure_ok) {
        scans = { 0, all_scans };
        for (size_t c = 0; c < nc; ++c) scans.push_back(1u << c);
    }
    for (unsigned m = 0; m <= all_maps; ++m)
        for (unsigned s : scans) {
            if (!m && !s) continue;
            point(m, s);
            one_case(0.5, b);
        }
}

void check_batches()
{
    for (int nq = 0; nq <= 3; ++nq) {
        int count[3] = { 0, 0, 0 };
        const int ncounts = nq == 0 ? 1 : nq == 1 ? 4 : nq == 2 ? 16 : 64;
        const int nperturb = nq == 0 ? 1 : nq == 1 ? 9 : nq == 2 ? 81 : 729;
        for (int ci = 0; ci < ncounts; ++ci) {
            int sum = 0;
            for (int q = 0, r = ci; q < nq; ++q, r /= 4) sum += count[q] = r % 4;
            for (int pi = 0; pi < nperturb; ++pi)
                for (int dd = -1; dd <= 1; ++dd) {
                    Batch b;
                    b.declared = sum + dd;
                    b.cs.assign((size_t)(b.declared > 0 ? b.declared : 0), lgs_loop_candidate{});
                    int first = 0;
                    for (int q = 0, r = pi; q < nq; ++q, r /= 9) {
                        lgs_loop_query Q{};
                        Q.first_candidate = first + r % 3 - 1;
                        Q.num_candidates = count[q] + r % 9 / 3 - 1;
                        first += count[q];
                        b.qs.push_back(Q);
                    }
                    cases_of(b);
                }
        }
    }
}

// fill_loop_result against memset + field assignments, InverseCompound inline.
void check_results()
{
    const lgs_pose2d poses[3] = { { 1.25, -0.5, 0.3 }, { -3.0, 2.0, -2.9 }, { 0.125, 7.5, 3.9 } };
    long long id = 0;
    for (const lgs_pose2d& node : poses)
        for (const lgs_pose2d& est : poses)
            for (int found = 0; found <= 1; ++found, ++id) {
                lgs_loop_query Q{};
                Q.local_map_node_pose = node;
                Q.local_map_node_index = 17;
                Q.first_candidate = 3;
                Q.num_candidates = 2;
                lgs_loop_candidate c{};
                c.node_pose = { 9.0, 9.0, 9.0 };
                c.node_index = 41;
                c.pad = 0x5a5a5a5a;
                lgs_rtcsm_summary s;
                std::memset(&s, 0x77, sizeof(s));
                s.pose_found = found;
                s.estimated_pose = est;
                s.score_max = 123.5;
                s.normalized_cost = 0.0625;
                for (int k = 0; k < 9; ++k) s.covariance[k] = 0.5 * k - 1.0;

                lgs_loop_result want;
                std::memset(&want, 0, sizeof(want));
                want.found = found;
                want.start_node_index = 17;
                want.end_node_index = 41;
                want.start_node_pose = node;
                want.estimated_pose = est;
                want.score = 123.5;
                want.normalized_cost = 0.0625;
                if (found) {
                    double sinT, cosT;
                    ::sincos(node.theta, &sinT, &cosT);
                    const double dx = est.x - node.x, dy = est.y - node.y;
                    want.relative_pose.x = cosT * dx + sinT * dy;
                    want.relative_pose.y = -sinT * dx + cosT * dy;
                    want.relative_pose.theta = est.theta - node.theta;
                }
                for (int k = 0; k < 9; ++k) want.covariance[k] = 0.5 * k - 1.0;

                lgs_loop_result got;
                std::memset(&got, 0xAB, sizeof(got));
                lgs::fill_loop_result(got, Q, c, s);
                if (std::memcmp(&got, &want, sizeof(want)) != 0) fail("loop result differs from the hand-built record", id);
                if (found) {
                    const lgs_pose2d rel = lgs::inverse_compound(node, est);
                    if (std::memcmp(&got.relative_pose, &rel, sizeof(rel)) != 0) fail("relative_pose", id);
                }
            }
}

}  // namespace

int main()
{
    static_assert(sizeof(lgs_loop_result) == 176, "lgs_loop_result is a fixed 176-byte record");
    check_batches();
    check_results();
    std::printf("%lld batches checked, %lld accepted\n", g_cases, g_accepted);
    if (g_failed || g_accepted == 0) {
        std::printf("%d LOOP HOST CHECKS FAILED\n", g_failed);
        return 1;
    }
    std::printf("LOOP HOST CHECKS PASSED\n");
    return 0;
}
