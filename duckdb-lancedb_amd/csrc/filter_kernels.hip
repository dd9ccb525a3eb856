// Filtered search on the device: the predicate program evaluator (one thread
// per slot, the interpreter of filter_program.h).  The bitmask-driven masked
// copy of the row terms (mask_rowaux_kernel) sits with the other row-term
// kernels in knn_kernels.hip.  Contract: knn_kernels.h; host side: index.h
// (Index::filter_begin, the filter cache).
#include <hip/hip_runtime.h>

#include "filter_program.h"
#include "knn_kernels.h"

namespace lhip {

// bits[w] bit l = live[64 w + l] && program TRUE for slot 64 w + l; slots past
// n_slots are 0.  One word per wavefront (wave64 ballot), one atomic per
// wavefront into *count.  The grid covers whole words: blockDim = 256 = 4 words.
__global__ __launch_bounds__(256) void filter_eval_kernel(const FpInstr *__restrict__ code, int n_code,
                                                          const uint64_t *__restrict__ lits,
                                                          const FpCol *__restrict__ cols,
                                                          const uint8_t *__restrict__ live, int64_t n_slots,
                                                          int64_t n_words, unsigned long long *__restrict__ bits,
                                                          unsigned long long *__restrict__ count) {
	const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
	bool t = false;
	if (r < n_slots && live[r]) t = fp_eval_row(code, n_code, lits, cols, r);
	const unsigned long long b = __ballot(t);
	const int64_t w = r >> 6;
	if ((threadIdx.x & 63) == 0 && w < n_words) {
		bits[w] = b;
		if (b) atomicAdd(count, (unsigned long long)__popcll(b));
	}
}

void launch_filter_eval(const void *code, int n_code, const uint64_t *lits, const void *cols, const uint8_t *live,
                        int64_t n_slots, uint64_t *bits, unsigned long long *count, hipStream_t st) {
	const int64_t n_words = (n_slots + 63) / 64;
	if (n_words <= 0) return;
	filter_eval_kernel<<<dim3((unsigned)((n_words + 3) / 4)), dim3(256), 0, st>>>(
	    static_cast<const FpInstr *>(code), n_code, lits, static_cast<const FpCol *>(cols), live, n_slots, n_words,
	    reinterpret_cast<unsigned long long *>(bits), count);
}

}  // namespace lhip
