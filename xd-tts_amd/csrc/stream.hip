// stream.hip -- the last stage of the delivery chain: the utterances of a sequence joined with their <break> silences into
// ONE stream, faded at their edges, levelled by one programme gain and encoded as fp32, PCM16 or G.711 mu-law / A-law (the
// definition: include/xdtts.h; the plan, the encoders and the walk of a pack: stream_plan.h).
// One kernel, k_stream_join, for xdtts_griffinlim_join and xdtts_synthesize_document in every format.  A workgroup owns
// STREAM_TILE_PACKS consecutive 16-byte packs of the OUTPUT stream; a lane takes pack lane, lane + 256, ... of the tile, so
// a wave's stores are 1 KiB contiguous.  The workgroup finds the utterance that owns its first sample once (bounded binary
// search on the exact 32-bit offsets) and keeps the STREAM_CACHE records from there in LDS; a tile that meets more falls back
// to the search in the table, sample by sample.  A pack inside one utterance reads 128 bits at a time where its source
// address allows, scalars otherwise; every pack but the stream's last, partial one leaves as one 128-bit store, and that one
// is written sample by sample: no byte at or behind total * sample_bytes is touched.
// One barrier behind the records, no exchange, no atomics, nothing from libm, no scratch: a byte of the output is a function
// of (inputs, plan, options) alone.
#include "kernels.h"

namespace xdtts {

namespace {

template <int FORMAT>
__device__ __forceinline__ void stream_tile(const StreamJob &J, void *__restrict__ out, const StreamUtt *cache, const StreamCache &c,
                                            uint32_t pack0, uint32_t n_packs) {
  constexpr int SB = FORMAT == STREAM_F32 ? 4 : (FORMAT == STREAM_PCM16 ? 2 : 1), P = STREAM_PACK_BYTES / SB;
#pragma unroll 1
  for (int s = 0; s < STREAM_STEPS; ++s) {
    const uint32_t pack = pack0 + (uint32_t)(s * STREAM_WG) + threadIdx.x;
    if (pack >= n_packs) return;
    uint32_t w[4];
    stream_pack<FORMAT>(J, cache, c, pack, w);
    const uint32_t k0 = pack * (uint32_t)P;
    if (k0 + (uint32_t)P <= J.total) {
      reinterpret_cast<uint4 *>(out)[pack] = make_uint4(w[0], w[1], w[2], w[3]);
      continue;
    }
    const int valid = (int)(J.total - k0);  // 1 .. P - 1: the stream's last pack
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (j >= valid) break;
      if (SB == 4) reinterpret_cast<uint32_t *>(out)[k0 + j] = w[j];
      else if (SB == 2) reinterpret_cast<uint16_t *>(out)[k0 + j] = (uint16_t)(w[j / 2] >> (16 * (j % 2)));
      else reinterpret_cast<uint8_t *>(out)[k0 + j] = (uint8_t)(w[j / 4] >> (8 * (j % 4)));
    }
  }
}

__global__ __launch_bounds__(STREAM_WG) void k_stream_join(StreamJob J, void *__restrict__ out) {
  __shared__ StreamUtt cache[STREAM_CACHE];
  const int SB = stream_sample_bytes(J.format), P = STREAM_PACK_BYTES / SB;
  const uint32_t n_packs = (J.total + (uint32_t)P - 1u) / (uint32_t)P;
  const uint32_t pack0 = blockIdx.x * (uint32_t)STREAM_TILE_PACKS;
  if (pack0 >= n_packs) return;  // (never: the host's grid)
  const StreamCache c = stream_cache_plan(J.tab, J.n_utt, pack0 * (uint32_t)P);  // (uniform: every lane reads the same records)
  if ((int)threadIdx.x < c.cnt) cache[threadIdx.x] = J.tab[c.u0 + (int)threadIdx.x];
  __syncthreads();
  switch (J.format) {  // (uniform)
    case STREAM_F32: stream_tile<STREAM_F32>(J, out, cache, c, pack0, n_packs); break;
    case STREAM_PCM16: stream_tile<STREAM_PCM16>(J, out, cache, c, pack0, n_packs); break;
    case STREAM_ULAW: stream_tile<STREAM_ULAW>(J, out, cache, c, pack0, n_packs); break;
    default: stream_tile<STREAM_ALAW>(J, out, cache, c, pack0, n_packs); break;
  }
}

}  // namespace

void launch_stream_join(const StreamJob &job, void *out, hipStream_t s) {
  if (job.total == 0 || job.total >= STREAM_TOTAL_MAX || job.n_utt < 1 || job.n_utt > STREAM_UTT_MAX || stream_sample_bytes(job.format) == 0 ||
      job.fade < 0 || job.fade > STREAM_FADE_MAX || (job.fade > 0 && !job.fade_tab))
    fail(XDTTS_ERR_BAD_ARG, "stream: %u samples, %d utterances, format %d, fade %d do not fit the kernel", job.total, job.n_utt, job.format,
         job.fade);
  hipLaunchKernelGGL(k_stream_join, dim3(stream_tiles(job.total, job.format)), dim3(STREAM_WG), 0, s, job, out);
  HIP_CHECK(hipGetLastError());
}

}  // namespace xdtts
