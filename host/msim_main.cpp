// msim_main.cpp — drop-in replacement for the reference's main.cpp driver on MI355X.
//
// Keeps the reference's configuration surface unchanged — SIM_DURATION (main.cpp:7), SIM_RUNS
// (main.cpp:10), SetupMiners() (main.cpp:44-65) with Miner(id, perc, propagation, selfish) — and its
// report (main.cpp:201, 219-234). The std::async batch loop (main.cpp:205-220) is replaced by
// msim_run_multi through the C ABI (include/msim.h): the runs are sharded over the GPUs, one stream
// per GPU, and combined by one RCCL all-reduce of the integer sums.
//
// Sweeps (BASELINE configs[3]) — the reference edits SetupMiners and rebuilds per network
// (README.md:21-27); here one invocation runs a whole grid or network list in one sweep launch per GPU
// (msim_sweep_run_multi) and prints main.cpp:224-234's report per point, or one JSON line per point:
//   msim_main [n_gpus] [seed_base] [default|c5]
//   msim_main --grid H1,H2,..:P1,P2,.. [--runs R] [--gpus N] [--seed S] [--json]
//        SetupMiners with miner 0 selfish at H% (miner 1 at 59-H%) and every propagation P ms
//   msim_main --sweep FILE.json [--runs R] [--gpus N] [--seed S] [--json] [--contrast P] [--shared-draws]
//        {"runs": R, "seed_base": S, "duration_ms": D, "total_weight": W,
//         "grid": {"selfish_perc": [..], "propagation_ms": [..]}}            or
//         "points": [{"miners": [{"id": 0, "perc": 40, "propagation_ms": 1000, "selfish": true}, ..]}, ..]}
//
// --errors (anywhere on the command line): per-miner standard errors from the exact on-device second moments
// (msim_run_moments / msim_sweep_run_moments, one GPU): " ± .." columns after each report line ("n/a" where a
// standard error is undefined, i.e. for a single run) and an "errors" object per miner in --json output.
// Without the flag the output is unchanged.
//
// --contrast P (sweeps; composes with --errors): every point against point P (from 0) on the same seeds, from the
// exact on-device cross sums (msim_sweep_run_contrasts, one GPU). After each other point's report lines one line
// per miner: its difference to the same miner of point P with the standard error of the per-run difference, the
// correlation of the two sides and the ratio; in --json output a "contrast" object per miner (msim_contrast's
// fields). P outside the points is a usage error.
//
// --classes (anywhere on the command line; composes with --errors, --json and --contrast): miners with equal
// (perc, propagation, selfish) form a class (for a sweep: by its first point's miners, one map for all points), and
// the exact on-device fold (msim_run_classes / msim_sweep_run_classes, one GPU) gives each class's found blocks,
// share and stale rate per run as ONE column, with standard errors. After a network's miner lines one line per
// class ("c5" gives three: the two pools and the 1 024 small miners); in --json output a "classes" array. With
// --contrast P the contrast lines are per class. For the plain driver --json prints the report as one JSON line
// and --runs R replaces SIM_RUNS.
//
// --quantiles Q1,Q2,.. (anywhere on the command line; composes with every other option): the exact quantiles of every
// miner's per-run found blocks, share and stale rate, selected on the device (msim_run_order_stats /
// msim_sweep_run_order_stats, one GPU, one more pass over the runs): the k-th smallest of the runs' values with
// k = max(1, ceil(q runs)). After a network's other lines one line per miner (per class with --classes, per point
// for a sweep); in --json output a "quantiles" object with the ranks and, per column and quantity (found, stale,
// share, rate; the last two in units of 2^-32), [value, below, equal] per rank.
//
// --tails Q (anywhere on the command line; composes with every other option): the lower tail of every miner's own
// share at the quantile Q (msim_run_tails / msim_sweep_run_tails, one GPU, one more pass over the runs): the blocks
// found, share and stale rate averaged over the miner's worst k = max(1, ceil(Q runs)) runs by share, ties at the
// quantile weighted equally, next to the all-runs means. One line per miner (per class with --classes, per point for
// a sweep); in --json output a "tails" object with the rank, k and per column a "tail" entry: the threshold, the run
// counts below and at it, the four tail means and the all-runs means.
//
// Build: make -C host
// "c5" runs BASELINE configs[4] (2 pools + 1 024 small miners, integer weights summing to
// W = 102 400, msim_config_create_weighted), which the reference's integer percentages cannot express.
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/msim.h"
#include "json_min.h"

using namespace std::chrono_literals;

//! How long to run each simulation for (main.cpp:7).
static constexpr std::chrono::months SIM_DURATION{12};
//! How many simulations to run (main.cpp:10).
static constexpr int SIM_RUNS{16 * 2'048};

struct Miner {  // simulation.h:57-59 constructor surface
    unsigned id;
    uint64_t perc;
    std::chrono::milliseconds propagation;
    bool is_selfish;
    Miner(unsigned id_, uint64_t perc_, std::chrono::milliseconds prop, bool selfish = false)
        : id{id_}, perc{perc_}, propagation{prop}, is_selfish{selfish} {}
};

/** Set the hashrate distribution for the simulation. Must add up to 100 (main.cpp:43-65). */
std::vector<Miner> SetupMiners()
{
    std::vector<Miner> miners;
    miners.emplace_back(0, 30, 1s);
    miners.emplace_back(1, 29, 1s);
    miners.emplace_back(2, 12, 1s);
    miners.emplace_back(3, 11, 1s);
    miners.emplace_back(4, 8, 1s);
    miners.emplace_back(5, 5, 1s);
    miners.emplace_back(6, 3, 1s);
    miners.emplace_back(7, 1, 1s);
    miners.emplace_back(8, 1, 1s);
    return miners;
}

/** The configs[3] grid network: SetupMiners with miner 0 selfish at h% and miner 1 at (59 - h)%, all at prop. */
std::vector<Miner> SetupSelfishMiners(uint64_t h, std::chrono::milliseconds prop)
{
    auto miners{SetupMiners()};
    miners[0].perc = h;
    miners[0].is_selfish = true;
    miners[1].perc = 59 - h;
    for (auto &m : miners) m.propagation = prop;
    return miners;
}

/** BASELINE configs[4] network: weights out of C5_TOTAL_WEIGHT, all honest, 1 s. */
static constexpr uint64_t C5_TOTAL_WEIGHT{102'400};
std::vector<Miner> SetupLargeNetwork()
{
    std::vector<Miner> miners;
    miners.emplace_back(0, 30'720, 1s);
    miners.emplace_back(1, 29'696, 1s);
    for (unsigned i = 0; i < 1'024; ++i) miners.emplace_back(2 + i, 41, 1s);
    return miners;
}

static int die(const char *what, int rc)
{
    std::fprintf(stderr, "%s: %s (%d)\n", what, msim_strerror(rc), rc);
    return 1;
}

// A standard error as the report prints its means (%g), "n/a" for NaN.
static std::string PlusMinus(double se, double scale, const char *unit)
{
    if (std::isnan(se)) return "n/a";
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%g%s", se * scale, unit);
    return buf;
}

// A number as the report prints its means (fmt: a printf format for one double), "n/a" for NaN.
static std::string Num(const char *fmt, double v, double scale = 1.0)
{
    if (std::isnan(v)) return "n/a";
    char buf[64];
    std::snprintf(buf, sizeof(buf), fmt, v * scale);
    return buf;
}

// The contrast lines of one point against point `baseline`, one per miner (contrasts.contrast_line in the package).
static void PrintContrasts(size_t point, size_t baseline, const msim_contrast *c, size_t m, const char *what = "Miner")
{
    for (size_t k = 0; k < m; ++k) {
        const msim_contrast &x = c[k];
        std::printf("  - %s %zu of point %zu vs point %zu: found %s ± %s blocks (corr %s), ×%s ± %s;"
                    " share %s ± %s of blocks (corr %s), ×%s ± %s; stale rate %s ± %s (corr %s)\n",
                    what, k, point, baseline, Num("%+g", x.found_diff).c_str(), Num("%g", x.found_diff_se).c_str(),
                    Num("%.3g", x.found_corr).c_str(), Num("%g", x.found_ratio).c_str(),
                    Num("%g", x.found_ratio_se).c_str(), Num("%+g%%", x.share_diff, 100.0).c_str(),
                    Num("%g%%", x.share_diff_se, 100.0).c_str(), Num("%.3g", x.share_corr).c_str(),
                    Num("%g", x.share_ratio).c_str(), Num("%g", x.share_ratio_se).c_str(),
                    Num("%+g%%", x.rate_diff, 100.0).c_str(), Num("%g%%", x.rate_diff_se, 100.0).c_str(),
                    Num("%.3g", x.rate_corr).c_str());
    }
}

// main.cpp:224-234 for one network; with `errors` (--errors) the standard errors of the three means follow each line.
static void PrintReport(const std::vector<Miner> &miners, const std::vector<msim_stats> &stats_total, uint64_t runs,
                        uint64_t total_weight, long long days, const msim_errors *errors = nullptr)
{
    std::printf("After running %llu simulations for %lldd each, on average:\n", (unsigned long long)runs, days);
    for (size_t i = 0; i < miners.size(); ++i) {
        const auto &miner{miners[i]};
        const auto &stats{stats_total[i]};
        if (total_weight == 100)
            std::printf("  - Miner %u (%llu%% of network hashrate) found %lld blocks i.e. ", miner.id,
                        (unsigned long long)miner.perc, (long long)(stats.blocks_found / (int64_t)runs));
        else
            std::printf("  - Miner %u (%g%% of network hashrate) found %lld blocks i.e. ", miner.id,
                        (double)miner.perc * 100.0 / (double)total_weight, (long long)(stats.blocks_found / (int64_t)runs));
        std::printf("%g%% of blocks. Stale rate: %g%%.", stats.blocks_share * 100 / (double)runs,
                    stats.stale_rate * 100 / (double)runs);
        if (miner.is_selfish) std::printf(" ('selfish mining' strategy)");
        if (errors)
            std::printf(" ± %s blocks, ± %s of blocks, stale rate ± %s", PlusMinus(errors[i].found_se, 1.0, "").c_str(),
                        PlusMinus(errors[i].share_se, 100.0, "%").c_str(), PlusMinus(errors[i].rate_se, 100.0, "%").c_str());
        std::printf("\n");
    }
}

// Miner classes (--classes): miners with equal (perc, propagation, selfish), numbered by first appearance.
struct Classes {
    std::vector<uint32_t> class_of;
    std::vector<uint32_t> members;   // per class
    std::vector<uint64_t> weight;    // per class: the sum of its members' perc
    uint32_t n() const { return (uint32_t)members.size(); }
};

static Classes GroupMiners(const std::vector<Miner> &miners)
{
    Classes c;
    std::vector<size_t> first;  // a member of each class
    for (size_t k = 0; k < miners.size(); ++k) {
        size_t at = 0;
        while (at < first.size() && !(miners[first[at]].perc == miners[k].perc &&
                                      miners[first[at]].propagation == miners[k].propagation &&
                                      miners[first[at]].is_selfish == miners[k].is_selfish))
            ++at;
        if (at == first.size()) {
            first.push_back(k);
            c.members.push_back(0);
            c.weight.push_back(0);
        }
        c.class_of.push_back((uint32_t)at);
        c.members[at] += 1;
        c.weight[at] += miners[k].perc;
    }
    return c;
}

// One line per class (classes.class_line in the package).
static void PrintClasses(const Classes &c, const msim_errors *e, uint64_t total_weight)
{
    for (uint32_t i = 0; i < c.n(); ++i)
        std::printf("  - Class %u (%u miners, %g%% of network hashrate) found %g ± %s blocks i.e. %g%% ± %s of blocks."
                    " Stale rate: %g%% ± %s.\n",
                    i, c.members[i], (double)c.weight[i] * 100.0 / (double)total_weight, e[i].found_mean,
                    PlusMinus(e[i].found_se, 1.0, "").c_str(), e[i].share_mean * 100,
                    PlusMinus(e[i].share_se, 100.0, "%").c_str(), e[i].rate_mean * 100,
                    PlusMinus(e[i].rate_se, 100.0, "%").c_str());
}

// --quantiles: the requested quantiles, their 0-based ranks among `runs` values, and msim_order_stat
// [point][column][4][rank] once selected (columns: miners, or classes with --classes).
struct Quantiles {
    std::vector<double> q;
    std::vector<uint64_t> ranks;
    std::vector<msim_order_stat> order;
    uint32_t cols = 0;
    bool on() const { return !q.empty(); }
    void SetRuns(uint64_t runs)
    {
        ranks.clear();
        for (double x : q) {
            const double k = std::ceil(x * (double)runs);  // hist_quantile's k
            ranks.push_back(k < 1.0 ? 0 : (uint64_t)k - 1);
        }
    }
    const msim_order_stat *at(size_t point, size_t col, size_t quantity) const
    {
        return order.data() + ((point * cols + col) * 4 + quantity) * ranks.size();
    }
};

static Quantiles ParseQuantiles(const std::string &s)
{
    Quantiles qs;
    std::stringstream ss(s);
    std::string tok;
    while (std::getline(ss, tok, ',')) {
        size_t used = 0;
        const double x = std::stod(tok, &used);
        if (used != tok.size() || !(x >= 0.0 && x <= 1.0)) throw std::runtime_error("--quantiles Q1,Q2,..: each within [0, 1]");
        qs.q.push_back(x);
    }
    if (qs.q.empty() || qs.q.size() > MSIM_MAX_RANKS)
        throw std::runtime_error("--quantiles Q1,Q2,..: 1 to " + std::to_string(MSIM_MAX_RANKS) + " quantiles");
    return qs;
}

// What follows a line's head (quantiles.quantile_columns in the package).
static void PrintQuantileColumns(const Quantiles &qs, size_t point, size_t col)
{
    static const char *const what[3] = {" blocks found: ", "; share of blocks: ", "; stale rate: "};
    static const size_t quantity[3] = {0, 2, 3};
    for (int w = 0; w < 3; ++w) {
        std::printf("%s", what[w]);
        const msim_order_stat *o = qs.at(point, col, quantity[w]);
        for (size_t j = 0; j < qs.q.size(); ++j) {
            std::printf("%sq%g = ", j ? ", " : "", qs.q[j]);
            if (w == 0)
                std::printf("%llu", (unsigned long long)o[j].value);
            else
                std::printf("%g%%", (double)o[j].value * 0x1.0p-32 * 100);
        }
    }
    std::printf(".\n");
}

// One line per miner, or per class (quantiles.report_quantiles in the package).
static void PrintQuantiles(const Quantiles &qs, size_t point, const std::vector<Miner> &miners, const Classes *classes,
                           uint64_t total_weight)
{
    for (size_t c = 0; c < qs.cols; ++c) {
        if (classes)
            std::printf("  - Class %zu (%u miners, %g%% of network hashrate)", c, classes->members[c],
                        (double)classes->weight[c] * 100.0 / (double)total_weight);
        else
            std::printf("  - Miner %u (%llu%% of network hashrate)", miners[c].id, (unsigned long long)miners[c].perc);
        PrintQuantileColumns(qs, point, c);
    }
}

static std::string JsonQuantiles(const Quantiles &qs, size_t point, bool classes)
{
    std::string s = ", \"quantiles\": {\"columns\": \"";
    s += classes ? "classes" : "miners";
    s += "\", \"q\": [";
    char buf[96];
    for (size_t j = 0; j < qs.q.size(); ++j) {
        std::snprintf(buf, sizeof(buf), "%s%.17g", j ? ", " : "", qs.q[j]);
        s += buf;
    }
    s += "], \"ranks\": [";
    for (size_t j = 0; j < qs.ranks.size(); ++j) s += (j ? ", " : "") + std::to_string(qs.ranks[j]);
    s += "], \"order\": [";
    for (size_t c = 0; c < qs.cols; ++c) {
        s += c ? ", [" : "[";
        for (size_t q = 0; q < 4; ++q) {
            s += q ? ", [" : "[";
            const msim_order_stat *o = qs.at(point, c, q);
            for (size_t j = 0; j < qs.ranks.size(); ++j) {
                std::snprintf(buf, sizeof(buf), "%s[%llu, %llu, %llu]", j ? ", " : "", (unsigned long long)o[j].value,
                              (unsigned long long)o[j].below, (unsigned long long)o[j].equal);
                s += buf;
            }
            s += "]";
        }
        s += "]";
    }
    return s + "]}";
}

// --tails Q: the lower tail of every column's own share at the quantile Q (msim_run_tails with one spec per column
// and point, each conditioned on itself): the order statistics, the columns' total moments and the tails,
// [point][column].
struct Tails {
    double q = -1.0;
    uint64_t rank = 0, runs = 0;
    uint32_t cols = 0;
    std::vector<msim_order_stat> order;  // [point][column][4][1]
    std::vector<msim_moments> total;
    std::vector<msim_tail> tails;
    std::vector<msim_tail_spec> specs;
    bool on() const { return q >= 0.0; }
    void Set(uint64_t n_runs, uint32_t columns, size_t points)
    {
        runs = n_runs;
        cols = columns;
        const double k = std::ceil(q * (double)n_runs);  // hist_quantile's k
        rank = k < 1.0 ? 0 : (uint64_t)k - 1;
        order.resize(points * cols * 4);
        total.resize(points * cols);
        tails.resize(points * cols);
        specs.clear();
        for (uint32_t p = 0; p < points; ++p)
            for (uint32_t c = 0; c < cols; ++c) specs.push_back({p, c, 2, 0, p, c});
    }
    // the means over the worst k = rank + 1 runs and over all runs of one column
    void Means(size_t point, size_t col, double mu[4], msim_errors *all) const
    {
        const size_t i = point * cols + col;
        if (msim_tail_means(&tails[i], &total[i], runs, rank + 1, 0, mu) != MSIM_OK) mu[0] = mu[1] = mu[2] = mu[3] = NAN;
        msim_moments_to_errors(&total[i], 1, runs, all);
    }
};

// One line per miner, or per class (tails.report_tails in the package; the text behind the head is
// tails.tail_columns).
static void PrintTails(const Tails &t, size_t point, const std::vector<Miner> &miners, const Classes *classes,
                       uint64_t total_weight)
{
    for (size_t c = 0; c < t.cols; ++c) {
        if (classes)
            std::printf("  - Class %zu (%u miners, %g%% of network hashrate)", c, classes->members[c],
                        (double)classes->weight[c] * 100.0 / (double)total_weight);
        else
            std::printf("  - Miner %u (%llu%% of network hashrate)", miners[c].id, (unsigned long long)miners[c].perc);
        double mu[4];
        msim_errors all;
        t.Means(point, c, mu, &all);
        std::printf(" in its worst %llu of %llu runs found %g blocks (all runs: %g) i.e. %g%% of blocks (%g%%)."
                    " Stale rate: %g%% (%g%%).\n",
                    (unsigned long long)(t.rank + 1), (unsigned long long)t.runs, mu[0], all.found_mean, mu[2] * 100,
                    all.share_mean * 100, mu[3] * 100, all.rate_mean * 100);
    }
}

static std::string JsonTails(const Tails &t, size_t point, bool classes)
{
    char buf[512];
    std::snprintf(buf, sizeof(buf), ", \"tails\": {\"columns\": \"%s\", \"q\": %.17g, \"rank\": %llu, \"k\": %llu, \"tail\": [",
                  classes ? "classes" : "miners", t.q, (unsigned long long)t.rank, (unsigned long long)(t.rank + 1));
    std::string s = buf;
    for (size_t c = 0; c < t.cols; ++c) {
        const size_t i = point * t.cols + c;
        double mu[4];
        msim_errors all;
        t.Means(point, c, mu, &all);
        std::snprintf(buf, sizeof(buf),
                      "%s{\"value\": %llu, \"n_below\": %llu, \"n_equal\": %llu, \"found\": %.17g, \"stale\": %.17g, "
                      "\"share\": %.17g, \"rate\": %.17g, \"all_runs\": {\"found\": %.17g, \"share\": %.17g, \"rate\": %.17g}}",
                      c ? ", " : "", (unsigned long long)t.order[i * 4 + 2].value, (unsigned long long)t.tails[i].n_below,
                      (unsigned long long)t.tails[i].n_equal, mu[0], mu[1], mu[2], mu[3], all.found_mean, all.share_mean,
                      all.rate_mean);
        s += buf;
    }
    return s + "]}";
}

// One JSON line for a point: the network and its per-miner averages (the report's numbers).
static void PrintJsonNumber(const char *sep, const char *name, double v)
{
    if (std::isnan(v))
        std::printf("%s\"%s\": null", sep, name);
    else
        std::printf("%s\"%s\": %.17g", sep, name, v);
}

static void PrintJsonErrors(const msim_errors &e)
{
    PrintJsonNumber("\"errors\": {", "found_mean", e.found_mean);
    PrintJsonNumber(", ", "found_se", e.found_se);
    PrintJsonNumber(", ", "share_mean", e.share_mean);
    PrintJsonNumber(", ", "share_se", e.share_se);
    PrintJsonNumber(", ", "rate_mean", e.rate_mean);
    PrintJsonNumber(", ", "rate_se", e.rate_se);
    PrintJsonNumber(", ", "pooled_rate", e.pooled_rate);
    PrintJsonNumber(", ", "pooled_rate_se", e.pooled_rate_se);
    std::printf("}");
}

static void PrintJsonContrast(const msim_contrast &c)
{
    const double *v = &c.found_diff;
    static const char *const names[16] = {
        "found_diff", "found_diff_se", "found_corr", "found_ratio", "found_ratio_se", "stale_diff",
        "stale_diff_se", "stale_corr", "share_diff", "share_diff_se", "share_corr", "share_ratio",
        "share_ratio_se", "rate_diff", "rate_diff_se", "rate_corr"};
    static_assert(sizeof(msim_contrast) == sizeof(double) * 16, "msim_contrast is 16 doubles");
    for (int f = 0; f < 16; ++f) PrintJsonNumber(f ? ", " : ", \"contrast\": {", names[f], v[f]);
    std::printf("}");
}

// With `classes` (--classes) a "classes" array follows the miners: per class its member count, hashrate, errors and,
// with class_contrast, its contrast against the baseline point; `contrast` is then per miner as without classes.
static void PrintJson(size_t point, const std::vector<Miner> &miners, const std::vector<msim_stats> &st, uint64_t runs,
                      uint64_t total_weight, const msim_errors *errors = nullptr, const msim_contrast *contrast = nullptr,
                      const Classes *classes = nullptr, const msim_errors *class_errors = nullptr,
                      const msim_contrast *class_contrast = nullptr, const std::string &tail = std::string())
{
    std::printf("{\"point\": %zu, \"runs\": %llu, \"total_weight\": %llu, \"miners\": [", point,
                (unsigned long long)runs, (unsigned long long)total_weight);
    for (size_t i = 0; i < miners.size(); ++i) {
        std::printf("%s{\"id\": %u, \"perc\": %llu, \"propagation_ms\": %lld, \"selfish\": %s, "
                    "\"blocks_found\": %.17g, \"blocks_share\": %.17g, \"stale_rate\": %.17g",
                    i ? ", " : "", miners[i].id, (unsigned long long)miners[i].perc,
                    (long long)miners[i].propagation.count(), miners[i].is_selfish ? "true" : "false",
                    (double)st[i].blocks_found / (double)runs, st[i].blocks_share / (double)runs,
                    st[i].stale_rate / (double)runs);
        if (errors) {
            std::printf(", ");
            PrintJsonErrors(errors[i]);
        }
        if (contrast) PrintJsonContrast(contrast[i]);
        std::printf("}");
    }
    std::printf("]");
    if (classes) {
        std::printf(", \"classes\": [");
        for (uint32_t c = 0; c < classes->n(); ++c) {
            std::printf("%s{\"class\": %u, \"members\": %u, \"hashrate_perc\": %.17g, ", c ? ", " : "", c,
                        classes->members[c], (double)classes->weight[c] * 100.0 / (double)total_weight);
            PrintJsonErrors(class_errors[c]);
            if (class_contrast) PrintJsonContrast(class_contrast[c]);
            std::printf("}");
        }
        std::printf("]");
    }
    std::printf("%s}\n", tail.c_str());  // --quantiles and --tails: their objects
}

// RCCL prints a version banner on stdout when a communicator is created. The report on stdout must keep
// main.cpp's exact format, so library output during the run call goes to stderr instead.
template <class F>
static int WithStdoutOnStderr(F f)
{
    std::fflush(stdout);
    const int saved = dup(1);
    if (saved >= 0) dup2(2, 1);
    const int rc = f();
    std::fflush(stdout);
    if (saved >= 0) {
        dup2(saved, 1);
        close(saved);
    }
    return rc;
}

static std::vector<msim_miner> Describe(const std::vector<Miner> &miners)
{
    std::vector<msim_miner> desc;
    for (const auto &m : miners)
        desc.push_back({m.id, m.perc, (int64_t)m.propagation.count(), (uint8_t)(m.is_selfish ? 1 : 0)});
    return desc;
}

static std::vector<int64_t> ParseList(const std::string &s)
{
    std::vector<int64_t> out;
    std::stringstream ss(s);
    std::string tok;
    while (std::getline(ss, tok, ',')) out.push_back(std::stoll(tok));
    return out;
}

struct SweepSpec {
    std::vector<std::vector<Miner>> points;
    uint64_t runs = 2'048;
    uint32_t seed_base = 1000;
    int64_t duration_ms = std::chrono::duration_cast<std::chrono::milliseconds>(SIM_DURATION).count();
    uint64_t total_weight = 100;
    int gpus = 1;
    bool json = false;
    bool errors = false;
    bool classes = false;  // --classes: statistics per class of identical miners (of the first point)
    Quantiles quantiles;   // --quantiles Q1,Q2,..
    Tails tails;           // --tails Q
    long long contrast = -1;  // --contrast P: the baseline point, or -1
    bool shared_draws = false;  // --shared-draws: msim_sweep_create_ex(MSIM_SWEEP_SHARED_DRAWS)
};

static void AddGrid(SweepSpec &sp, const std::vector<int64_t> &hs, const std::vector<int64_t> &props)
{
    for (int64_t h : hs)
        for (int64_t p : props) sp.points.push_back(SetupSelfishMiners((uint64_t)h, std::chrono::milliseconds{p}));
}

static SweepSpec LoadSweepFile(const std::string &path)
{
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::stringstream buf;
    buf << f.rdbuf();
    const std::string text = buf.str();
    const jmin::Value root = jmin::Parser(text).parse();
    SweepSpec sp;
    if (const auto *v = root.get("runs")) sp.runs = (uint64_t)v->as_int();
    if (const auto *v = root.get("seed_base")) sp.seed_base = (uint32_t)v->as_int();
    if (const auto *v = root.get("duration_ms")) sp.duration_ms = v->as_int();
    if (const auto *v = root.get("total_weight")) sp.total_weight = (uint64_t)v->as_int();
    if (const auto *v = root.get("gpus")) sp.gpus = (int)v->as_int();
    if (const auto *g = root.get("grid")) {
        std::vector<int64_t> hs, ps;
        for (const auto &x : g->get("selfish_perc")->arr) hs.push_back(x.as_int());
        for (const auto &x : g->get("propagation_ms")->arr) ps.push_back(x.as_int());
        AddGrid(sp, hs, ps);
    }
    if (const auto *pts = root.get("points")) {
        for (const auto &pt : pts->arr) {
            std::vector<Miner> ms;
            for (const auto &m : pt.get("miners")->arr) {
                const auto *sel = m.get("selfish");
                ms.emplace_back((unsigned)m.get("id")->as_int(), (uint64_t)m.get("perc")->as_int(),
                                std::chrono::milliseconds{m.get("propagation_ms")->as_int()}, sel && sel->as_bool());
            }
            sp.points.push_back(std::move(ms));
        }
    }
    if (sp.points.empty()) throw std::runtime_error("no points in " + path);
    return sp;
}

static int RunSweep(const SweepSpec &sp)
{
    std::vector<msim_config *> cfgs;
    int rc = MSIM_OK;
    for (const auto &pt : sp.points) {
        const auto desc{Describe(pt)};
        msim_config *c = nullptr;
        rc = msim_config_create_weighted(desc.data(), (uint32_t)desc.size(), sp.duration_ms, sp.total_weight, &c);
        if (rc) break;
        cfgs.push_back(c);
    }
    msim_sweep *sw = nullptr;
    if (rc == MSIM_OK) rc = msim_sweep_create_ex(cfgs.data(), (uint32_t)cfgs.size(), sp.shared_draws ? MSIM_SWEEP_SHARED_DRAWS : 0u, &sw);
    const uint32_t m = cfgs.empty() ? 0 : msim_config_miner_count(cfgs[0]);
    std::vector<msim_stats> st(sp.points.size() * m);
    std::vector<msim_errors> errs;
    std::vector<msim_contrast> con;  // [point != baseline, in order][miner], or [class] with --classes
    Classes cls;
    std::vector<msim_errors> cerrs;  // [point][class]
    if (rc == MSIM_OK && sp.classes) {
        cls = GroupMiners(sp.points[0]);
        const uint32_t nc = cls.n();
        std::vector<msim_pair> pairs;
        for (uint32_t p = 0; p < sp.points.size() && sp.contrast >= 0; ++p)
            for (uint32_t c = 0; c < nc && p != (uint32_t)sp.contrast; ++c) pairs.push_back({p, c, (uint32_t)sp.contrast, c});
        std::vector<msim_moments> cmo(sp.points.size() * nc), mo(sp.errors ? st.size() : 0);
        std::vector<msim_cross> cross(pairs.size());
        rc = WithStdoutOnStderr([&] {
            return msim_sweep_run_classes(sw, 0, sp.runs, sp.seed_base, 0, cls.class_of.data(), nc,
                                          pairs.empty() ? nullptr : pairs.data(), (uint32_t)pairs.size(), st.data(),
                                          nullptr, cmo.data(), nullptr, nullptr, pairs.empty() ? nullptr : cross.data());
        });
        if (rc == MSIM_OK && sp.errors)  // the miners' own standard errors need the miners' moments: a second pass
            rc = WithStdoutOnStderr([&] {
                return msim_sweep_run_moments(sw, 0, sp.runs, sp.seed_base, 0, st.data(), nullptr, mo.data(), nullptr, nullptr);
            });
        if (rc == MSIM_OK) {
            cerrs.resize(cmo.size());
            msim_moments_to_errors(cmo.data(), (uint32_t)cmo.size(), sp.runs, cerrs.data());
            con.resize(pairs.size());
            if (!pairs.empty())
                msim_cross_to_contrasts(cmo.data(), nc, pairs.data(), cross.data(), (uint32_t)pairs.size(), sp.runs, con.data());
            if (sp.errors) {
                errs.resize(st.size());
                msim_moments_to_errors(mo.data(), (uint32_t)mo.size(), sp.runs, errs.data());
            }
        }
    } else if (rc == MSIM_OK && sp.contrast >= 0) {
        std::vector<msim_pair> pairs;
        for (uint32_t p = 0; p < sp.points.size(); ++p)
            for (uint32_t k = 0; k < m && p != (uint32_t)sp.contrast; ++k) pairs.push_back({p, k, (uint32_t)sp.contrast, k});
        std::vector<msim_moments> mo(st.size());
        std::vector<msim_cross> cross(pairs.size());
        if (!pairs.empty())
            rc = WithStdoutOnStderr([&] {
                return msim_sweep_run_contrasts(sw, 0, sp.runs, sp.seed_base, 0, pairs.data(), (uint32_t)pairs.size(),
                                                st.data(), nullptr, mo.data(), cross.data());
            });
        else  // a single point has nothing to be compared with
            rc = WithStdoutOnStderr([&] {
                return msim_sweep_run_moments(sw, 0, sp.runs, sp.seed_base, 0, st.data(), nullptr, mo.data(), nullptr, nullptr);
            });
        if (rc == MSIM_OK) {
            con.resize(pairs.size());
            msim_cross_to_contrasts(mo.data(), m, pairs.data(), cross.data(), (uint32_t)pairs.size(), sp.runs, con.data());
            if (sp.errors) {
                errs.resize(st.size());
                msim_moments_to_errors(mo.data(), (uint32_t)mo.size(), sp.runs, errs.data());
            }
        }
    } else if (rc == MSIM_OK && sp.errors) {
        std::vector<msim_moments> mo(st.size());
        errs.resize(st.size());
        rc = WithStdoutOnStderr([&] {
            return msim_sweep_run_moments(sw, 0, sp.runs, sp.seed_base, 0, st.data(), nullptr, mo.data(), nullptr, nullptr);
        });
        if (rc == MSIM_OK) msim_moments_to_errors(mo.data(), (uint32_t)mo.size(), sp.runs, errs.data());
    } else if (rc == MSIM_OK) {
        rc = WithStdoutOnStderr([&] {
            return msim_sweep_run_multi(sw, 0, sp.runs, sp.seed_base, nullptr, (uint32_t)sp.gpus, st.data(), nullptr);
        });
    }
    Quantiles qs = sp.quantiles;
    if (rc == MSIM_OK && qs.on()) {  // one more pass over the runs: every point's records stay on the device
        if (sp.classes && cls.class_of.empty()) cls = GroupMiners(sp.points[0]);
        qs.SetRuns(sp.runs);
        qs.cols = sp.classes ? cls.n() : m;
        qs.order.resize(sp.points.size() * qs.cols * 4 * qs.ranks.size());
        std::vector<msim_stats> again(st.size());
        rc = WithStdoutOnStderr([&] {
            return msim_sweep_run_order_stats(sw, 0, sp.runs, sp.seed_base, 0, sp.classes ? cls.class_of.data() : nullptr,
                                              sp.classes ? cls.n() : 0, qs.ranks.data(), (uint32_t)qs.ranks.size(),
                                              again.data(), nullptr, qs.order.data());
        });
    }
    Tails tl = sp.tails;
    if (rc == MSIM_OK && tl.on()) {  // and one for the tails: the selection, then the tail launches on the same records
        if (sp.classes && cls.class_of.empty()) cls = GroupMiners(sp.points[0]);
        tl.Set(sp.runs, sp.classes ? cls.n() : m, sp.points.size());
        std::vector<msim_stats> again(st.size());
        rc = WithStdoutOnStderr([&] {
            return msim_sweep_run_tails(sw, 0, sp.runs, sp.seed_base, 0, sp.classes ? cls.class_of.data() : nullptr,
                                        sp.classes ? cls.n() : 0, &tl.rank, 1, tl.specs.data(), (uint32_t)tl.specs.size(),
                                        again.data(), nullptr, tl.order.data(), tl.total.data(), tl.tails.data());
        });
    }
    if (rc == MSIM_OK) {
        const long long days = sp.duration_ms / 86'400'000;
        for (size_t p = 0; p < sp.points.size(); ++p) {
            const std::vector<msim_stats> ps(st.begin() + p * m, st.begin() + (p + 1) * m);
            const msim_errors *pe = sp.errors ? errs.data() + p * m : nullptr;
            const msim_contrast *pc = nullptr;
            const size_t cols = sp.classes ? cls.n() : m;  // columns of a point's contrasts
            if (sp.contrast >= 0 && p != (size_t)sp.contrast && !con.empty())
                pc = con.data() + (p - (p > (size_t)sp.contrast)) * cols;
            const msim_errors *ce = sp.classes ? cerrs.data() + p * cls.n() : nullptr;
            if (sp.json) {
                const std::string tail = (qs.on() ? JsonQuantiles(qs, p, sp.classes) : std::string()) +
                                         (tl.on() ? JsonTails(tl, p, sp.classes) : std::string());
                if (sp.classes)
                    PrintJson(p, sp.points[p], ps, sp.runs, sp.total_weight, pe, nullptr, &cls, ce, pc, tail);
                else
                    PrintJson(p, sp.points[p], ps, sp.runs, sp.total_weight, pe, pc, nullptr, nullptr, nullptr, tail);
            } else {
                std::printf("Point %zu of %zu:\n", p + 1, sp.points.size());
                PrintReport(sp.points[p], ps, sp.runs, sp.total_weight, days, pe);
                if (sp.classes) PrintClasses(cls, ce, sp.total_weight);
                if (pc) PrintContrasts(p, (size_t)sp.contrast, pc, cols, sp.classes ? "Class" : "Miner");
                if (qs.on()) PrintQuantiles(qs, p, sp.points[p], sp.classes ? &cls : nullptr, sp.total_weight);
                if (tl.on()) PrintTails(tl, p, sp.points[p], sp.classes ? &cls : nullptr, sp.total_weight);
            }
        }
    }
    if (sw) msim_sweep_destroy(sw);
    for (auto *c : cfgs) msim_config_destroy(c);
    return rc;
}

int main(int argc, char **argv)
{
    bool errors = false;   // --errors, wherever it stands; the other arguments keep their positions
    bool classes = false;  // --classes, likewise
    Quantiles quantiles;   // --quantiles Q1,Q2,.., likewise
    Tails tails;           // --tails Q, likewise
    {
        int kept = 1;
        for (int i = 1; i < argc; ++i) {
            if (std::string(argv[i]) == "--quantiles" && i + 1 < argc) {
                try {
                    quantiles = ParseQuantiles(argv[++i]);
                } catch (const std::exception &e) {
                    std::fprintf(stderr, "msim_main: %s\n", e.what());
                    return 2;
                }
            } else if (std::string(argv[i]) == "--tails" && i + 1 < argc) {
                char *end = nullptr;
                tails.q = std::strtod(argv[++i], &end);
                if (end == argv[i] || *end || !(tails.q >= 0.0 && tails.q <= 1.0)) {
                    std::fprintf(stderr, "msim_main: --tails Q: Q within [0, 1]\n");
                    return 2;
                }
            } else if (std::string(argv[i]) == "--errors")
                errors = true;
            else if (std::string(argv[i]) == "--classes")
                classes = true;
            else
                argv[kept++] = argv[i];
        }
        argc = kept;
    }
    if (argc > 1 && (std::string(argv[1]) == "--grid" || std::string(argv[1]) == "--sweep")) {
        SweepSpec sp;
        try {
            if (argc < 3) throw std::runtime_error("missing argument");
            if (std::string(argv[1]) == "--sweep") {
                sp = LoadSweepFile(argv[2]);
            } else {
                const std::string g = argv[2];
                const size_t colon = g.find(':');
                if (colon == std::string::npos) throw std::runtime_error("--grid H1,H2,..:P1,P2,..");
                AddGrid(sp, ParseList(g.substr(0, colon)), ParseList(g.substr(colon + 1)));
            }
            for (int i = 3; i < argc; ++i) {
                const std::string a = argv[i];
                if (a == "--json") sp.json = true;
                else if (a == "--shared-draws") sp.shared_draws = true;
                else if (a == "--runs" && i + 1 < argc) sp.runs = std::stoull(argv[++i]);
                else if (a == "--gpus" && i + 1 < argc) sp.gpus = std::stoi(argv[++i]);
                else if (a == "--seed" && i + 1 < argc) sp.seed_base = (uint32_t)std::stoul(argv[++i]);
                else if (a == "--contrast" && i + 1 < argc) {
                    sp.contrast = std::stoll(argv[++i]);
                    if (sp.contrast < 0) throw std::runtime_error("--contrast P: P is a point, from 0");
                }
                else throw std::runtime_error("unknown option " + a);
            }
            sp.errors = errors;
            sp.classes = classes;
            sp.quantiles = quantiles;
            sp.tails = tails;
            if (sp.contrast >= (long long)sp.points.size())
                throw std::runtime_error("--contrast " + std::to_string(sp.contrast) + ": there are " +
                                         std::to_string(sp.points.size()) + " points");
        } catch (const std::exception &e) {
            std::fprintf(stderr, "msim_main: %s\n", e.what());
            return 2;
        }
        if (int rc = RunSweep(sp)) return die("sweep", rc);
        return 0;
    }
    // the plain driver: --json and --runs R wherever they stand, then the positional arguments
    bool json = false;
    uint64_t sim_runs = SIM_RUNS;
    {
        int kept = 1;
        for (int i = 1; i < argc; ++i) {
            if (std::string(argv[i]) == "--json")
                json = true;
            else if (std::string(argv[i]) == "--runs" && i + 1 < argc)
                sim_runs = std::strtoull(argv[++i], nullptr, 10);
            else
                argv[kept++] = argv[i];
        }
        argc = kept;
        if (sim_runs == 0) {
            std::fprintf(stderr, "msim_main: --runs R: R is at least 1\n");
            return 2;
        }
    }
    const bool large = argc > 3 && std::string(argv[3]) == "c5";
    const auto miners{large ? SetupLargeNetwork() : SetupMiners()};
    const uint64_t total_weight = large ? C5_TOTAL_WEIGHT : 100;
    const int n_gpus = argc > 1 ? std::atoi(argv[1]) : 1;
    const int64_t duration_ms = std::chrono::duration_cast<std::chrono::milliseconds>(SIM_DURATION).count();
    const uint32_t seed_base = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 1000u;

    const auto desc{Describe(miners)};
    msim_config *cfg = nullptr;
    if (int rc = msim_config_create_weighted(desc.data(), (uint32_t)desc.size(), duration_ms, total_weight, &cfg))
        return die("config", rc);

    // main.cpp:201 (the reference names its thread count; here one stream drives each GPU)
    if (!json) std::printf("Running %llu simulations in parallel using %d threads.\n", (unsigned long long)sim_runs, n_gpus);
    std::vector<msim_stats> stats_total(miners.size());
    std::vector<msim_errors> errs, cerrs;
    Classes cls;
    if (classes) {
        cls = GroupMiners(miners);
        std::vector<msim_moments> cmo(cls.n());
        cerrs.resize(cls.n());
        if (int rc = WithStdoutOnStderr([&] {
                return msim_run_classes(cfg, 0, sim_runs, seed_base, 0, cls.class_of.data(), cls.n(), nullptr, 0,
                                        stats_total.data(), nullptr, cmo.data(), nullptr, nullptr, nullptr);
            }))
            return die("msim_run_classes", rc);
        msim_moments_to_errors(cmo.data(), cls.n(), sim_runs, cerrs.data());
    }
    // with --classes and --errors the miners' own standard errors need the miners' moments: a second pass
    if (errors) {
        std::vector<msim_moments> mo(miners.size());
        errs.resize(miners.size());
        if (int rc = WithStdoutOnStderr([&] {
                return msim_run_moments(cfg, 0, sim_runs, seed_base, 0, stats_total.data(), nullptr, mo.data(), nullptr,
                                        nullptr);
            }))
            return die("msim_run_moments", rc);
        msim_moments_to_errors(mo.data(), (uint32_t)mo.size(), sim_runs, errs.data());
    } else if (!classes) {
        if (int rc = WithStdoutOnStderr([&] {
                return msim_run_multi(cfg, 0, sim_runs, seed_base, nullptr, (uint32_t)n_gpus, stats_total.data(), nullptr);
            }))
            return die("msim_run_multi", rc);
    }
    if (quantiles.on()) {  // one more pass over the runs: their records stay on the device
        quantiles.SetRuns(sim_runs);
        quantiles.cols = classes ? cls.n() : (uint32_t)miners.size();
        quantiles.order.resize((size_t)quantiles.cols * 4 * quantiles.ranks.size());
        std::vector<msim_stats> again(miners.size());
        if (int rc = WithStdoutOnStderr([&] {
                return msim_run_order_stats(cfg, 0, sim_runs, seed_base, 0, classes ? cls.class_of.data() : nullptr,
                                            classes ? cls.n() : 0, quantiles.ranks.data(), (uint32_t)quantiles.ranks.size(),
                                            again.data(), nullptr, quantiles.order.data());
            }))
            return die("msim_run_order_stats", rc);
    }
    if (tails.on()) {  // and one for the tails
        tails.Set(sim_runs, classes ? cls.n() : (uint32_t)miners.size(), 1);
        std::vector<msim_stats> again(miners.size());
        if (int rc = WithStdoutOnStderr([&] {
                return msim_run_tails(cfg, 0, sim_runs, seed_base, 0, classes ? cls.class_of.data() : nullptr,
                                      classes ? cls.n() : 0, &tails.rank, 1, tails.specs.data(), (uint32_t)tails.specs.size(),
                                      again.data(), nullptr, tails.order.data(), tails.total.data(), tails.tails.data());
            }))
            return die("msim_run_tails", rc);
    }
    if (json) {
        PrintJson(0, miners, stats_total, sim_runs, total_weight, errors ? errs.data() : nullptr, nullptr,
                  classes ? &cls : nullptr, classes ? cerrs.data() : nullptr, nullptr,
                  (quantiles.on() ? JsonQuantiles(quantiles, 0, classes) : std::string()) +
                      (tails.on() ? JsonTails(tails, 0, classes) : std::string()));
        msim_config_destroy(cfg);
        return 0;
    }
    std::printf("\r100%% progress..\n");  // main.cpp:219-221

    const auto days{std::chrono::duration_cast<std::chrono::days>(SIM_DURATION)};
    PrintReport(miners, stats_total, sim_runs, total_weight, (long long)days.count(), errors ? errs.data() : nullptr);
    if (classes) PrintClasses(cls, cerrs.data(), total_weight);
    if (quantiles.on()) PrintQuantiles(quantiles, 0, miners, classes ? &cls : nullptr, total_weight);
    if (tails.on()) PrintTails(tails, 0, miners, classes ? &cls : nullptr, total_weight);
    msim_config_destroy(cfg);
    return 0;
}
