// A variable-length bit stream put together by a whole workgroup in LDS: what png_deflate_pack_kernel and
// jpeg_code_kernel share.  The `image` is an array of 32-bit words of LDS that stands for the words w0, w0 + 1, .. of the
// stream; threads OR their codes into it (LDS integer or: order-free, so the bytes do not depend on which thread comes
// first), and once per pass the complete words leave through a caller-supplied sink while the open word is carried into
// the next pass.  A pass of the caller:
//     barrier                      every put of the pass is in the image             (the caller's)
//     refid_bits_retire            complete words -> sink, ONE barrier inside, image[0] = the open word, the rest zero
//     barrier                      the image is ready for the next puts              (the caller's; any barrier between the
//                                  retire and the next put will do, the two of refid_block_scan included)
//     refid_block_scan of the threads' bit counts -> every thread's position `at`, cursor += total
//     RefidBitWriter<ORDER> w(at); w.put(image, code, nbits) ..; w.flush(image)
//
// Bit order is a property of the format: REFID_BITS_LSB_FIRST (deflate) fills a word from bit 0 up, and the words are the
// stream's bytes as a little-endian machine stores them; REFID_BITS_MSB_FIRST (JPEG) fills from bit 31 down, and a word is
// byte-swapped when it leaves.
#pragma once
#include <hip/hip_runtime.h>
#include "workgroup.h"

enum RefidBitOrder { REFID_BITS_LSB_FIRST, REFID_BITS_MSB_FIRST };

// One thread's run of consecutive codes, starting at bit `at` of the image.  Up to 63 bits wait in `acc`; a finished word
// is OR-ed into the image, and so is what is left at the flush unless it is all zeros (the image starts out zero).  put:
// 1 <= nbits <= 32, and v has no bits above nbits.  flush: once, after the last put.
template <RefidBitOrder ORDER>
struct RefidBitWriter {
    unsigned long long acc;
    unsigned filled, word;

    __device__ __forceinline__ explicit RefidBitWriter(unsigned at) : acc(0ull), filled(at & 31u), word(at >> 5) {}

    __device__ __forceinline__ unsigned head() const { return ORDER == REFID_BITS_LSB_FIRST ? (unsigned)acc : (unsigned)(acc >> 32); }

    __device__ __forceinline__ void flush(unsigned* image) const {
        if (head()) atomicOr(&image[word], head());
    }
    __device__ __forceinline__ void put(unsigned* image, unsigned v, unsigned nbits) {
        acc |= ORDER == REFID_BITS_LSB_FIRST ? (unsigned long long)v << filled : (unsigned long long)v << (64u - filled - nbits);
        filled += nbits;
        if (filled >= 32u) {
            atomicOr(&image[word], head());
            acc = ORDER == REFID_BITS_LSB_FIRST ? acc >> 32 : acc << 32;
            filled -= 32u, ++word;
        }
    }
};

// a single code at bit `at` of the image
template <RefidBitOrder ORDER>
__device__ __forceinline__ void refid_bits_put_at(unsigned* image, unsigned at, unsigned v, unsigned nbits) {
    RefidBitWriter<ORDER> w(at);
    w.put(image, v, nbits);
    w.flush(image);
}

// The image's words [0, n) go to sink(w0 + i, image[i]), each from one thread.  No barrier.
template <int THREADS, class Sink>
__device__ __forceinline__ void refid_bits_drain(const unsigned* image, int n, int w0, Sink&& sink) {
    for (int i = threadIdx.x; i < n; i += THREADS) sink(w0 + i, image[i]);
}

// The retire step of a pass.  cursor: bits of the stream so far (counted from word 0); w0: the stream word that image[0]
// stands for.  The complete words [0, n_full) drain to the sink, the open word image[n_full] becomes image[0], the words
// [1, n_full] -- all that the pass could have touched -- are zeroed, and w0 advances by n_full.
// Barriers: ONE inside, between the reads of the image and its rewrite.  The caller has a barrier behind its last put
// before the call, and one between the call and its next put (see the pass above).
template <int THREADS, class Sink>
__device__ __forceinline__ void refid_bits_retire(unsigned* image, unsigned cursor, int& w0, Sink&& sink) {
    const int n_full = (int)(cursor >> 5) - w0;
    const unsigned carry = image[n_full];
    refid_bits_drain<THREADS>(image, n_full, w0, sink);
    __syncthreads();
    for (int i = threadIdx.x; i <= n_full; i += THREADS) image[i] = i == 0 ? carry : 0u;
    w0 += n_full;
}

// The walk of an offsets kernel: one workgroup lays n records end to end.  Thread t takes the ceil(n / THREADS)
// consecutive records from t * ceil(n / THREADS) on ([lo, hi), as refid_chunk gives them), adds up length(j) over them, a
// workgroup scan turns that into the offset of its first record, and it hands every record to store(j, offset, total):
// offset = the sum of the lengths of the records before j, total = the sum of all.  length(j) is called twice per record
// and must give the same value both times.  red: THREADS / 64 words of LDS; the barriers are those of refid_block_scan.
template <int THREADS>
__device__ __forceinline__ void refid_chunk(int n, int* lo, int* hi) {
    const int per = (n + THREADS - 1) / THREADS;
    *lo = min((int)threadIdx.x * per, n), *hi = min(*lo + per, n);      // (tid * per < 2^31: per <= 2^23)
}
template <int THREADS, class Length, class Store>
__device__ __forceinline__ unsigned refid_chunk_offsets(int n, unsigned* red, Length&& length, Store&& store) {
    int lo, hi;
    refid_chunk<THREADS>(n, &lo, &hi);
    unsigned mine = 0;
    for (int j = lo; j < hi; ++j) mine += length(j);
    unsigned total = 0;
    unsigned off = refid_block_scan<THREADS / 64>(mine, red, &total);
    for (int j = lo; j < hi; ++j) {
        store(j, off, total);
        off += length(j);
    }
    return total;
}
