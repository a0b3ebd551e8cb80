// ragged_layout.h -- the host half of a batch of ragged utterances (the kernels' half: ragged_batch.h): the check of
// the offset arrays a host entry is given, before they reach the device.  The kernels take everything in those arrays
// on trust, so this is all that stands between a caller's offsets and reads or writes outside the buffers.
// Host only and free of HIP: a plain C++ compiler builds it (tests/ragged_layout_selftest.cpp does).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace jdsp {

enum class RaggedVerdict { kOk, kFirstNotZero, kDecreasing, kSampleParity, kOverlap, kPastEnd };

struct RaggedLayout {
    RaggedVerdict verdict = RaggedVerdict::kOk;
    int64_t end = 0;        // one past the last sample of the last span: nothing behind it is read or written
    int64_t n_total = 0;    // unit_first[n_utts]: the frames (blocks) of the whole batch
    int64_t longest = 0;    // the largest count of one utterance
};

// Utterance u is the units (frames or blocks) unit_first[u] .. unit_first[u + 1] - 1 and starts at sample
// sample_first[u] of n_samples; f > 0 units span hop (f - 1) + n samples, none span none (blocks of hop samples:
// n = hop; hop > 0).  The first check that fails is the verdict: unit_first[0] is 0; then, utterance by utterance in
// this order, unit_first does not decrease; sample_first is even and >= 0; the span starts at or behind the end of
// the one before; it ends at or before n_samples.  No expression here overflows, whatever the arrays hold: a count is
// the difference of two values already known to be >= 0 and ordered, and a span is measured against the room that is
// left, never added up first.  Neither array is read for n_utts <= 0.
inline RaggedLayout ragged_layout_check(const int64_t *sample_first, const int64_t *unit_first, int64_t n_utts,
                                        int64_t n_samples, int64_t n, int64_t hop)
{
    RaggedLayout r;
    const auto bad = [&r](RaggedVerdict v) { r.verdict = v; return r; };
    if (n_utts > 0 && unit_first[0] != 0) return bad(RaggedVerdict::kFirstNotZero);
    for (int64_t u = 0; u < n_utts; u++) {
        if (unit_first[u + 1] < unit_first[u]) return bad(RaggedVerdict::kDecreasing);
        const int64_t f = unit_first[u + 1] - unit_first[u], s = sample_first[u];
        if (s < 0 || (s & 1)) return bad(RaggedVerdict::kSampleParity);
        if (s < r.end) return bad(RaggedVerdict::kOverlap);
        if (s > n_samples || (f > 0 && (n_samples - s < n || f - 1 > (n_samples - s - n) / hop)))
            return bad(RaggedVerdict::kPastEnd);
        r.end = f > 0 ? s + hop * (f - 1) + n : s;
        if (f > r.longest) r.longest = f;
    }
    if (n_utts > 0) r.n_total = unit_first[n_utts];
    return r;
}

// The message of a failed check as the entry `entry` reports it; axis names its unit array ("frame_first",
// "block_first").  Empty for kOk.
inline std::string ragged_layout_message(RaggedVerdict v, const char *entry, const char *axis)
{
    const std::string e = std::string(entry) + ": ", a(axis);
    switch (v) {
    case RaggedVerdict::kOk: break;
    case RaggedVerdict::kFirstNotZero: return e + a + "[0] must be 0";
    case RaggedVerdict::kDecreasing: return e + a + " must not decrease";
    case RaggedVerdict::kSampleParity: return e + "sample_first entries must be even and >= 0";
    case RaggedVerdict::kOverlap: return e + "sample_first must ascend and the utterances' spans must not overlap";
    case RaggedVerdict::kPastEnd: return e + "an utterance's span ends past n_samples";
    }
    return std::string();
}

// ---- live streams: the stream ids that come with a list of chunks (or of streams to flush) -------------------------
enum class StreamIdVerdict { kOk, kRange, kDuplicate };

// Every id in [0, n_streams) and no id twice: a kernel indexes the handle's tails by them, and two chunks of one stream
// in a call would both start from the same tail.  The first id that fails is the verdict, range before duplicate.
inline StreamIdVerdict stream_ids_check(const int64_t *stream_id, int64_t n_ids, int64_t n_streams)
{
    if (n_ids <= 0) return StreamIdVerdict::kOk;
    std::vector<int64_t> sorted(stream_id, stream_id + n_ids);
    for (int64_t id : sorted)
        if (id < 0 || id >= n_streams) return StreamIdVerdict::kRange;
    std::sort(sorted.begin(), sorted.end());
    return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end() ? StreamIdVerdict::kOk
                                                                            : StreamIdVerdict::kDuplicate;
}

inline std::string stream_ids_message(StreamIdVerdict v, const char *entry)
{
    const std::string e = std::string(entry) + ": ";
    switch (v) {
    case StreamIdVerdict::kOk: break;
    case StreamIdVerdict::kRange: return e + "a stream id lies outside [0, n_streams)";
    case StreamIdVerdict::kDuplicate: return e + "a stream id occurs twice";
    }
    return std::string();
}

}  // namespace jdsp
