// channels.hip -- the channels of an interleaved recording as planes:
//     out[j * out_pitch + i] = in[i * channels + select[j]]        i < nframes, j < nselect
// Samples are moved as bytes (4, 2 or 1 per sample), never converted.  The selection rides in the kernel's argument block
// (64 bytes), so a launch uploads nothing and is legal under stream capture.  HBM-bound by construction: channels * nframes
// samples are read once, nselect * nframes written.
//
// Two forms in ONE launch (the channel entries add one kernel to the batch entry's count):
//   * stereo (channels == 2), where the host found source and destination aligned for it: a lane loads 16 contiguous bytes of
//     interleaved data per instruction -- 1 KiB per wavefront instruction --, four such loads in flight before the first store,
//     separates left and right in registers and stores 8 contiguous bytes per selected channel and load.  A block's loads and
//     stores go through buffer descriptors over what is left of the aligned run, so the last block is range-checked by the
//     hardware and the run need not be a whole number of blocks.
//   * general (any channel count, any alignment; the few sample frames in front of and behind the aligned run of the stereo
//     form): a lane per sample frame, a loop over the selected channels with sample-sized loads and stores.  Consecutive lanes
//     hold consecutive sample frames, so a wavefront's loads cover one contiguous span of the recording.
// The first `wide_blocks` blocks of a launch run the stereo form over sample frames [wide_lo, wide_lo + wide_n), the rest the
// general form over the frames outside that range.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glfer {

struct ChannelArgs {
  const void *in;
  void *out;
  unsigned long long nframes, out_pitch;           // sample frames; samples from one plane to the next
  unsigned long long wide_lo, wide_n;              // the stereo form's run (wide_n: a multiple of a lane's 8 / ESZ sample frames)
  unsigned wide_blocks;
  int channels, nselect;
  unsigned select[16];                             // nselect bytes, four to a word
};

__device__ __forceinline__ unsigned selected(const ChannelArgs &a, int j) { return (a.select[j >> 2] >> ((j & 3) * 8)) & 0xffu; }

template <int ESZ> struct SampleBits;
template <> struct SampleBits<4> { typedef uint32_t type; };
template <> struct SampleBits<2> { typedef uint16_t type; };
template <> struct SampleBits<1> { typedef uint8_t type; };

typedef unsigned v4u32 __attribute__((ext_vector_type(4)));
typedef unsigned v2u32 __attribute__((ext_vector_type(2)));

// 16 interleaved bytes (L R L R ...) -> the 8 bytes of channel `right`
template <int ESZ>
__device__ __forceinline__ v2u32 one_of_two(v4u32 q, unsigned right) {
  if constexpr (ESZ == 4) {
    return right ? v2u32{q.y, q.w} : v2u32{q.x, q.z};
  } else if constexpr (ESZ == 2) {
    return right ? v2u32{(q.x >> 16) | (q.y & 0xffff0000u), (q.z >> 16) | (q.w & 0xffff0000u)}
                 : v2u32{(q.x & 0xffffu) | (q.y << 16), (q.z & 0xffffu) | (q.w << 16)};
  } else {
    auto half = [&](unsigned d) { return right ? ((d >> 8) & 0xffu) | ((d >> 16) & 0xff00u) : (d & 0xffu) | ((d >> 8) & 0xff00u); };
    return v2u32{half(q.x) | (half(q.y) << 16), half(q.z) | (half(q.w) << 16)};
  }
}

template <int ESZ>
__global__ __launch_bounds__(256) void deinterleave_kernel(const ChannelArgs a) {
  typedef typename SampleBits<ESZ>::type T;
  const unsigned t = threadIdx.x;
  if (blockIdx.x < a.wide_blocks) {
    constexpr unsigned FPL = 8 / ESZ, LOADS = 4;                               // sample frames per lane and load; loads in flight
    constexpr unsigned long long FPB = 256ull * LOADS * FPL;                    // sample frames per block
    const unsigned long long f0 = (unsigned long long)blockIdx.x * FPB;         // the block's first frame of the run
    const unsigned long long left = a.wide_n - f0;                              // frames of the run from there (> 0: the launcher's grid)
    const unsigned nfr = (unsigned)(left < FPB ? left : FPB);
    const __amdgpu_buffer_rsrc_t src = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char *>(static_cast<const char *>(a.in)) + (a.wide_lo + f0) * (2ull * ESZ), 0, nfr * 2u * ESZ, 0x00020000);
    v4u32 q[LOADS];
#pragma unroll
    for (unsigned k = 0; k < LOADS; k++) q[k] = __builtin_amdgcn_raw_buffer_load_b128(src, (k * 256u + t) * 16u, 0u, 0);
    for (int j = 0; j < a.nselect; j++) {
      const unsigned right = selected(a, j) & 1u;
      const __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc(
          static_cast<char *>(a.out) + ((unsigned long long)j * a.out_pitch + a.wide_lo + f0) * ESZ, 0, nfr * ESZ, 0x00020000);
#pragma unroll
      for (unsigned k = 0; k < LOADS; k++) __builtin_amdgcn_raw_buffer_store_b64(one_of_two<ESZ>(q[k], right), dst, (k * 256u + t) * 8u, 0u, 0);
    }
    return;
  }
  // the general form: leftover frame r of the launch is frame r below the stereo run, r + wide_n above it
  const unsigned long long r = (unsigned long long)(blockIdx.x - a.wide_blocks) * 256ull + t;
  const unsigned long long i = r < a.wide_lo ? r : r + a.wide_n;
  if (i >= a.nframes) return;
  const T *in = static_cast<const T *>(a.in) + i * (unsigned long long)a.channels;
  T *out = static_cast<T *>(a.out) + i;
  int j = 0;
  for (; j + 4 <= a.nselect; j += 4) {                                          // four loads in flight, then their stores
    T v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = in[selected(a, j + k)];
#pragma unroll
    for (int k = 0; k < 4; k++) out[(unsigned long long)(j + k) * a.out_pitch] = v[k];
  }
  for (; j < a.nselect; j++) out[(unsigned long long)j * a.out_pitch] = in[selected(a, j)];
}

}  // namespace glfer

using namespace glfer;

// select: nselect channel indices below `channels`, 1 <= nselect <= 64 (the caller has checked them); esz: 4, 2 or 1.
// wide: 0 keeps the general form everywhere (A/B runs and tests); otherwise the stereo form runs where channels == 2 and the
// pointers and the pitch allow it.
extern "C" hipError_t glfer_launch_deinterleave(const void *in, size_t nframes, int channels, int esz, const unsigned char *select,
                                                int nselect, void *out, size_t out_pitch, int wide, hipStream_t st) {
  if (nframes == 0) return hipSuccess;
  if (channels < 1 || channels > 64 || nselect < 1 || nselect > 64 || (esz != 4 && esz != 2 && esz != 1)) return hipErrorInvalidValue;
  ChannelArgs a = {};
  a.in = in;
  a.out = out;
  a.nframes = nframes;
  a.out_pitch = out_pitch;
  a.channels = channels;
  a.nselect = nselect;
  for (int j = 0; j < nselect; j++) a.select[j >> 2] |= (unsigned)select[j] << ((j & 3) * 8);
  const size_t fpl = 8 / (size_t)esz, fpb = 256 * 4 * fpl;
  if (wide && channels == 2) {
    // the first sample frame whose two samples start a 16-byte line of the source; the same frame must sit on an 8-byte
    // boundary of every plane written
    const uintptr_t s = reinterpret_cast<uintptr_t>(in), d = reinterpret_cast<uintptr_t>(out);
    const size_t off = (16 - s % 16) % 16;
    if (off % (2 * (size_t)esz) == 0) {
      const size_t i0 = off / (2 * (size_t)esz);
      const bool dst_ok = (d + i0 * (size_t)esz) % 8 == 0 && (nselect == 1 || (out_pitch * (size_t)esz) % 8 == 0);
      if (dst_ok && nframes > i0) {
        a.wide_lo = i0;
        a.wide_n = (nframes - i0) / fpl * fpl;
      }
    }
  }
  const size_t wide_blocks = (a.wide_n + fpb - 1) / fpb, rest = nframes - a.wide_n, blocks = wide_blocks + (rest + 255) / 256;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  a.wide_blocks = (unsigned)wide_blocks;
  switch (esz) {
    case 4: hipLaunchKernelGGL((deinterleave_kernel<4>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    case 2: hipLaunchKernelGGL((deinterleave_kernel<2>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((deinterleave_kernel<1>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
  }
  return hipGetLastError();
}
