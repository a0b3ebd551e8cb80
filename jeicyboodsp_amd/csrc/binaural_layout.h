// binaural_layout.h -- the host half of a binaural delivery (the kernels' half: binaural_kernels.hip): the check of
// the arrays jdsp_binaural_render is given, before they reach the device.  The render kernel takes everything in them
// on trust (it only clamps dir and the stream ids into range), so this is what stands between a caller's arrays and
// reads or writes outside the buffers.  Host only and free of HIP: a plain C++ compiler builds it.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "ragged_layout.h"

namespace jdsp {

struct BinauralDelivery {
    const int64_t *stream_id, *sample_first;   // [n_chunks]
    const int32_t *dir;                        // [n_chunks]
    const float *gain;                         // [n_chunks]
    const int64_t *chunk_first, *block_first;  // [n_mixes + 1]
    int64_t n_mixes, n_chunks, n_samples, plane;
    bool has_output;                           // out_i16 or out_f32 is given
};

constexpr int64_t kBinauralBlock = 512;
constexpr int64_t kBinauralMaxBlocks = 0x3ffffff0;     // blocks of one delivery: the render kernel's grid

// Empty: the delivery is sound, and n_blocks_total = block_first[n_mixes] (0 for no mixes).  Otherwise what is wrong
// with it, the first check that fails, in the order: counts; both *_first arrays start at 0, do not decrease, and
// chunk_first ends at n_chunks; ids in range and distinct; per chunk dir in range, gain finite, sample_first even and
// >= 0, its 512 B_m samples inside n_samples; the output blocks inside plane.  Input spans may coincide or overlap:
// they are only read.  No expression overflows, whatever the arrays hold.
inline std::string binaural_delivery_check(const BinauralDelivery &d, int64_t n_streams, int64_t n_dirs,
                                           int64_t *n_blocks_total)
{
    *n_blocks_total = 0;
    if (d.n_mixes < 0 || d.n_chunks < 0 || d.n_samples < 0) return "n_mixes, n_chunks or n_samples < 0";
    if (d.plane < 0 || (d.plane & 1)) return "plane must be even and >= 0";
    if (d.n_chunks > n_streams) return "more chunks than live streams (ids are distinct within a call)";
    if (d.n_mixes == 0) return d.n_chunks ? "chunks without a mix" : "";
    if (!d.chunk_first || !d.block_first) return "chunk_first or block_first is NULL";
    if (d.n_chunks && (!d.stream_id || !d.sample_first || !d.dir || !d.gain))
        return "stream_id, sample_first, dir or gain is NULL";
    if (d.chunk_first[0] != 0) return "chunk_first[0] must be 0";
    if (d.block_first[0] != 0) return "block_first[0] must be 0";
    for (int64_t m = 0; m < d.n_mixes; m++) {
        if (d.chunk_first[m + 1] < d.chunk_first[m]) return "chunk_first must not decrease";
        if (d.block_first[m + 1] < d.block_first[m]) return "block_first must not decrease";
    }
    if (d.chunk_first[d.n_mixes] != d.n_chunks) return "chunk_first[n_mixes] must be n_chunks";
    if (d.block_first[d.n_mixes] > kBinauralMaxBlocks) return "more than 2^30 - 16 blocks in one delivery";
    const StreamIdVerdict v = stream_ids_check(d.stream_id, d.n_chunks, n_streams);
    if (v == StreamIdVerdict::kRange) return "a stream id lies outside [0, n_streams)";
    if (v == StreamIdVerdict::kDuplicate) return "a stream id occurs twice";
    for (int64_t m = 0; m < d.n_mixes; m++) {
        const int64_t blocks = d.block_first[m + 1] - d.block_first[m];
        for (int64_t c = d.chunk_first[m]; c < d.chunk_first[m + 1]; c++) {
            if (d.dir[c] < 0 || d.dir[c] >= n_dirs) return "a dir lies outside [0, n_dirs)";
            if (!std::isfinite(d.gain[c])) return "a gain is not finite";
            const int64_t s = d.sample_first[c];
            if (s < 0 || (s & 1)) return "sample_first entries must be even and >= 0";
            if (s > d.n_samples || blocks > (d.n_samples - s) / kBinauralBlock) return "a chunk's span ends past n_samples";
        }
    }
    if (d.has_output && d.block_first[d.n_mixes] > d.plane / kBinauralBlock) return "the output blocks do not fit in plane";
    *n_blocks_total = d.block_first[d.n_mixes];
    return "";
}

}  // namespace jdsp
