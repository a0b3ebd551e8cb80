// ragged_layout_selftest.cpp -- csrc/ragged_layout.h against the loop it replaced, on the host alone.  Built by
// tests/test_ragged_layout_cpu.py with the host compiler under AddressSanitizer and UndefinedBehaviorSanitizer (no
// recovery): a read past an offset array or a signed overflow inside the check ends the program with a report.
//   1. a seeded sweep of small layouts, most of them valid, half of them poked: verdict, end and n_total equal the
//      transcribed loop's, and the sweep is shown not to be vacuous (every verdict occurs often enough);
//   2. boundary cases by hand, with the inputs on which the old loop itself overflowed;
//   3. every message, for both axis names, against the literal text.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../jeicyboodsp_amd/csrc/ragged_layout.h"

using jdsp::RaggedLayout;
using jdsp::RaggedVerdict;

static int g_bad = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED line %d: %s\n", __LINE__, #cond);                 \
            g_bad++;                                                         \
        }                                                                    \
    } while (0)

// ---- the reference: the check of jdsp_stftmask_batch as it stood before ragged_layout.h, word for word from
// "everything the kernel takes on trust" to n_total; fail() here only keeps the message ---------------------------
namespace ref {

struct Ctx { std::string error; };
constexpr int JDSP_OK = 0, JDSP_EINVAL = -1;
static int fail(Ctx *ctx, int code, const char *what)
{
    ctx->error = what;
    return code;
}

static int stftmask_batch_check(Ctx *ctx, const long n, const long hop, long n_samples, const int64_t *sample_first_host,
                                const int64_t *frame_first_host, long n_utts, long *end_out, long *n_total_out)
{
    // everything the kernel takes on trust from device-side offsets is checked here
    if (n_utts > 0 && frame_first_host[0] != 0) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_batch: frame_first[0] must be 0");
    long end = 0;                                              // one past the last sample of the spans so far
    for (long u = 0; u < n_utts; u++) {
        const long f = frame_first_host[u + 1] - frame_first_host[u], s = sample_first_host[u];
        if (f < 0) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_batch: frame_first must not decrease");
        if (s < 0 || (s & 1)) return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_batch: sample_first entries must be even and >= 0");
        if (s < end)
            return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_batch: sample_first must ascend and the utterances' spans must not overlap");
        if (s > n_samples || (f > 0 && (n_samples - s < n || f - 1 > (n_samples - s - n) / hop)))
            return fail(ctx, JDSP_EINVAL, "jdsp_stftmask_batch: an utterance's span ends past n_samples");
        end = f > 0 ? s + hop * (f - 1) + n : s;
    }
    const long n_total = n_utts > 0 ? frame_first_host[n_utts] : 0;
    *end_out = end, *n_total_out = n_total;
    return JDSP_OK;
}

}  // namespace ref

// in the enum's order
static const char *const kVerdictNames[6] = {"accepted", "first not 0", "decreasing", "parity/sign", "overlap", "past the end"};

// ---- 1. the sweep -----------------------------------------------------------------------------------------------
static void sweep()
{
    static const long kGeom[6][2] = {{1024, 1024}, {1024, 512}, {1024, 256}, {512, 256}, {512, 128}, {512, 512}};
    const int kCases = 20000;
    std::mt19937_64 rng(20261019);
    const auto below = [&rng](uint64_t m) { return (long)(rng() % m); };
    long seen[6] = {0, 0, 0, 0, 0, 0};
    int mismatches = 0;
    for (int c = 0; c < kCases; c++) {
        const long n = kGeom[c % 6][0], hop = kGeom[c % 6][1];
        const long n_utts = below(7);
        // exactly sized, so that a read past either array is AddressSanitizer's to report
        std::vector<int64_t> sample((size_t)n_utts), first((size_t)n_utts + 1);
        long pos = 0;
        first[0] = 0;
        for (long u = 0; u < n_utts; u++) {
            const long f = below(4) == 0 ? 0 : below(5);
            sample[u] = pos;
            first[u + 1] = first[u] + f;
            pos += (f > 0 ? hop * (f - 1) + n : 0) + 2 * below(4);     // the span, then an even gap of 0 .. 6
        }
        long n_samples = pos;
        if (below(2)) {                                                // one poke
            const long kind = below(3);
            if (kind == 0 && n_utts > 0) {
                static const long kDelta[6] = {1, -1, 2, -2, 0, 0};
                const long d = below(6);
                sample[below(n_utts)] += d == 4 ? hop : d == 5 ? -hop : kDelta[d];
            } else if (kind == 1) {
                first[below(n_utts + 1)] += below(2) ? 1 : -1;
            } else {
                n_samples -= below(2) ? 2 : hop;
            }
        }
        ref::Ctx ctx;
        long end = -1, n_total = -1;
        const int rc = ref::stftmask_batch_check(&ctx, n, hop, n_samples, sample.data(), first.data(), n_utts, &end, &n_total);
        const RaggedLayout got = jdsp::ragged_layout_check(sample.data(), first.data(), n_utts, n_samples, n, hop);
        const std::string msg = jdsp::ragged_layout_message(got.verdict, "jdsp_stftmask_batch", "frame_first");
        bool same = (rc == ref::JDSP_OK) == (got.verdict == RaggedVerdict::kOk) && msg == ctx.error;
        if (same && rc == ref::JDSP_OK) same = got.end == end && got.n_total == n_total;
        if (!same && mismatches++ < 5)
            printf("case %d (n %ld hop %ld utts %ld): reference '%s' end %ld total %ld, got '%s' end %lld total %lld\n", c, n,
                   hop, n_utts, ctx.error.c_str(), end, n_total, msg.c_str(), (long long)got.end, (long long)got.n_total);
        if (same) seen[(int)got.verdict]++;                            // the reference's verdict too
    }
    CHECK(mismatches == 0);
    printf("sweep of %d layouts:", kCases);
    for (int v = 0; v < 6; v++) printf(" %s %ld%s", kVerdictNames[v], seen[v], v < 5 ? "," : "\n");
    // not vacuous: mostly valid layouts, and every rejection often enough to mean something
    CHECK(seen[0] >= kCases * 40 / 100 && seen[0] <= kCases * 90 / 100);
    for (int v = 1; v < 6; v++) CHECK(seen[v] >= kCases / 100);
}

// ---- 2. boundary cases ------------------------------------------------------------------------------------------
static void boundaries()
{
    const int64_t kMin = INT64_MIN, kMax = INT64_MAX;
    {   // a span that ends exactly at n_samples, and one sample short of it
        const int64_t s[2] = {0, 2050}, f[3] = {0, 2, 5};              // 1536 from 0; 2048 from 2050: ends at 4098
        RaggedLayout r = jdsp::ragged_layout_check(s, f, 2, 4098, 1024, 512);
        CHECK(r.verdict == RaggedVerdict::kOk && r.end == 4098 && r.n_total == 5 && r.longest == 3);
        r = jdsp::ragged_layout_check(s, f, 2, 4097, 1024, 512);
        CHECK(r.verdict == RaggedVerdict::kPastEnd);
        // blocks (n = hop): 3 and 5 blocks of 512
        const int64_t sb[2] = {0, 1538}, fb[3] = {0, 3, 8};
        r = jdsp::ragged_layout_check(sb, fb, 2, 1538 + 2560, 512, 512);
        CHECK(r.verdict == RaggedVerdict::kOk && r.end == 4098 && r.n_total == 8 && r.longest == 5);
        r = jdsp::ragged_layout_check(sb, fb, 2, 1538 + 2559, 512, 512);
        CHECK(r.verdict == RaggedVerdict::kPastEnd);
    }
    {   // no utterance: neither array is read
        const RaggedLayout r = jdsp::ragged_layout_check(nullptr, nullptr, 0, 0, 1024, 512);
        CHECK(r.verdict == RaggedVerdict::kOk && r.end == 0 && r.n_total == 0 && r.longest == 0);
    }
    {   // only empty utterances, all at the same offset
        const int64_t s[3] = {6, 6, 6}, f[4] = {0, 0, 0, 0};
        RaggedLayout r = jdsp::ragged_layout_check(s, f, 3, 6, 1024, 256);
        CHECK(r.verdict == RaggedVerdict::kOk && r.end == 6 && r.n_total == 0 && r.longest == 0);
        r = jdsp::ragged_layout_check(s, f, 3, 4, 1024, 256);          // ... but not behind the buffer's end
        CHECK(r.verdict == RaggedVerdict::kPastEnd);
    }
    {   // the subtraction the old loop began with overflows here
        const int64_t s[2] = {0, 1024}, f[3] = {0, 1, kMin};
        const RaggedLayout r = jdsp::ragged_layout_check(s, f, 2, 4096, 1024, 512);
        CHECK(r.verdict == RaggedVerdict::kDecreasing);
    }
    {
        const int64_t f[2] = {0, 1};
        int64_t s[1] = {kMin};
        CHECK(jdsp::ragged_layout_check(s, f, 1, 4096, 1024, 512).verdict == RaggedVerdict::kSampleParity);
        s[0] = kMax - 1;
        CHECK(jdsp::ragged_layout_check(s, f, 1, 4096, 1024, 512).verdict == RaggedVerdict::kPastEnd);
        s[0] = 0;
        const RaggedLayout r = jdsp::ragged_layout_check(s, f, 1, kMax, 1024, 512);
        CHECK(r.verdict == RaggedVerdict::kOk && r.end == 1024 && r.n_total == 1);
        const int64_t huge[2] = {0, kMax};                             // more frames than any buffer holds
        CHECK(jdsp::ragged_layout_check(s, huge, 1, kMax, 1024, 512).verdict == RaggedVerdict::kPastEnd);
    }
}

// ---- 3. the messages --------------------------------------------------------------------------------------------
static void messages()
{
    using jdsp::ragged_layout_message;
    const auto is = [](RaggedVerdict v, const char *entry, const char *axis, const char *want) {
        return ragged_layout_message(v, entry, axis) == want;
    };
    CHECK(is(RaggedVerdict::kFirstNotZero, "jdsp_istft_batch", "frame_first", "jdsp_istft_batch: frame_first[0] must be 0"));
    CHECK(is(RaggedVerdict::kDecreasing, "jdsp_istft_batch", "frame_first", "jdsp_istft_batch: frame_first must not decrease"));
    CHECK(is(RaggedVerdict::kSampleParity, "jdsp_stft_half_batch", "frame_first",
             "jdsp_stft_half_batch: sample_first entries must be even and >= 0"));
    CHECK(is(RaggedVerdict::kOverlap, "jdsp_stftmask_batch", "frame_first",
             "jdsp_stftmask_batch: sample_first must ascend and the utterances' spans must not overlap"));
    CHECK(is(RaggedVerdict::kPastEnd, "jdsp_stftmask_batch", "frame_first",
             "jdsp_stftmask_batch: an utterance's span ends past n_samples"));
    CHECK(is(RaggedVerdict::kFirstNotZero, "jdsp_denoise_batch", "block_first", "jdsp_denoise_batch: block_first[0] must be 0"));
    CHECK(is(RaggedVerdict::kDecreasing, "jdsp_denoise_batch", "block_first", "jdsp_denoise_batch: block_first must not decrease"));
    CHECK(is(RaggedVerdict::kSampleParity, "jdsp_denoise_batch", "block_first",
             "jdsp_denoise_batch: sample_first entries must be even and >= 0"));
    CHECK(is(RaggedVerdict::kOverlap, "jdsp_denoise_batch", "block_first",
             "jdsp_denoise_batch: sample_first must ascend and the utterances' spans must not overlap"));
    CHECK(is(RaggedVerdict::kPastEnd, "jdsp_denoise_batch", "block_first",
             "jdsp_denoise_batch: an utterance's span ends past n_samples"));
    CHECK(is(RaggedVerdict::kOk, "jdsp_denoise_batch", "block_first", ""));
}

int main()
{
    sweep();
    boundaries();
    messages();
    if (g_bad) {
        printf("ragged layout: %d checks FAILED\n", g_bad);
        return 1;
    }
    printf("ragged layout: ok\n");
    return 0;
}
