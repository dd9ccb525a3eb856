// gfx950 kernels of the IVF_SQ index (ivf.h has the numerics contract, DESIGN.md
// "IVF_SQ" the layout): 8-bit scalar-quantised rows in list order, scanned by
// v_mfma_i32_16x16x64_i8 against int8 queries.
//
// Stands in for what rust_lib/src/lance_manager.rs:517-551 builds behind
// lance_detached_create_hnsw_index (IvfHnswSqIndexBuilder: IVF partitions over
// scalar-quantised rows, an HNSW graph per partition): the probed partitions are
// scanned whole by the SQ distance, so the graph's ranking without its misses.
//   build   sq_minmax (bounds lo / hi of the k-means sample) -> at layout time
//           sq_encode (codes c' = c - 128 and the L2 row term, list order)
//   search  sq_query_prep (int8 queries, (sq s, sq mid sum qi) pairs) ->
//           sq_list_scan (256 positions x 16 probing queries per MFMA tile,
//           per-wave sorted runs of SQ keys) -> ivf_merge -> exact re-rank
#include "ivf.h"
#include "device_common.h"

#include <stdexcept>

namespace lhip {

namespace {

constexpr uint64_t SQ_KEY_NONE = ~0ull;
constexpr int SQ_G = 16;         // queries per MFMA column block
constexpr int SQ_KROW = 257;     // u64 stride of a query's 256 keys in LDS (bank spread)

// f32 steps rounded one at a time (the numpy reference's order): operators
// created under contract(off) never fuse into v_fmac
__device__ __forceinline__ float add_nc(float a, float b) {
#pragma clang fp contract(off)
	return a + b;
}
__device__ __forceinline__ float sub_nc(float a, float b) {
#pragma clang fp contract(off)
	return a - b;
}
__device__ __forceinline__ float mul_nc(float a, float b) {
#pragma clang fp contract(off)
	return a * b;
}
__device__ __forceinline__ uint64_t key64(float d, uint32_t slot) { return ((uint64_t)fkey(d) << 32) | slot; }

// ascending bitonic sort of one 64-bit key per lane across the wave (no LDS, no barrier)
__device__ __forceinline__ uint64_t wave_sort64(uint64_t k) {
	const int lane = threadIdx.x & 63;
#pragma unroll
	for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
		for (int stride = size >> 1; stride > 0; stride >>= 1) {
			const uint64_t o = __shfl_xor(k, stride, 64);
			const bool asc = (lane & size) == 0, lower = (lane & stride) == 0;
			k = (lower == asc) ? (o < k ? o : k) : (o > k ? o : k);
		}
	}
	return k;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

}  // namespace

// ---------------------------------------------------------------------------
// build: bounds of the training sample
// ---------------------------------------------------------------------------
// out[0] = min, out[1] = max of fkey(v) over the dim real elements of n rows
// (stride ld); NaN elements are skipped.  out must be pre-set to (~0, 0).
__global__ __launch_bounds__(256) void sq_minmax_kernel(const float *__restrict__ S, int64_t n, int ld, int dim,
                                                        uint32_t *__restrict__ out) {
	__shared__ uint32_t smin[4], smax[4];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t lo = 0xFFFFFFFFu, hi = 0u;
	for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < n; r += (int64_t)gridDim.x * 4) {
		const float *x = S + r * ld;
		for (int i = lane; i < dim; i += 64) {
			const float v = x[i];
			if (v != v) continue;
			const uint32_t k = fkey(v);
			lo = min(lo, k);
			hi = max(hi, k);
		}
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		lo = min(lo, (uint32_t)__shfl_xor((int)lo, o, 64));
		hi = max(hi, (uint32_t)__shfl_xor((int)hi, o, 64));
	}
	if (lane == 0) {
		smin[w] = lo;
		smax[w] = hi;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		atomicMin(out, min(min(smin[0], smin[1]), min(smin[2], smin[3])));
		atomicMax(out + 1, max(max(smax[0], smax[1]), max(smax[2], smax[3])));
	}
}

void launch_sq_minmax(const float *S, int64_t n, int ld, int dim, uint32_t *out, hipStream_t st) {
	HIPCHK(hipMemsetAsync(out, 0xFF, sizeof(uint32_t), st));
	HIPCHK(hipMemsetAsync(out + 1, 0, sizeof(uint32_t), st));
	if (n <= 0) return;
	const unsigned grid = (unsigned)std::min<int64_t>((n + 3) / 4, 4096);
	sq_minmax_kernel<<<dim3(grid), 256, 0, st>>>(S, n, ld, dim, out);
}

// ---------------------------------------------------------------------------
// encode: one wave per output row
// ---------------------------------------------------------------------------
// Row p of the output is the row of slot lslot[p] (slot p when lslot is null):
// c = clamp(rint((v - lo) / s), 0, 255), v = x or x * (1 / |x|) (cosine: the row
// aux scale), written as c - shift at out + p * ldo for the dim real elements
// and 0 for the elements dim .. padto; SLOT_NONE rows are all zero.  rt (when
// non-null) gets the L2 row term from the exact integer sums of c' = c - 128.
template <typename T>
__global__ __launch_bounds__(256) void sq_encode_kernel(const T *__restrict__ X, int ld, int dim,
                                                        const float *__restrict__ rowaux_f, int normalize,
                                                        const uint32_t *__restrict__ lslot, int64_t npos, float lo,
                                                        float s, float mid, int shift, int ldo, int padto,
                                                        uint8_t *__restrict__ out, float *__restrict__ rt) {
	const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	const int lane = threadIdx.x & 63;
	if (p >= npos) return;
	const uint32_t slot = lslot ? lslot[p] : (uint32_t)p;
	uint8_t *o = out + p * (int64_t)ldo;
	if (slot == SLOT_NONE) {
		for (int i = lane; i < padto; i += 64) o[i] = 0;
		if (rt && lane == 0) rt[p] = 0.0f;
		return;
	}
	const T *x = X + (int64_t)slot * ld;
	const float sc = normalize ? rowaux_f[raix(slot, 3)] : 1.0f;
	int s1 = 0;
	long long s2 = 0;
	for (int i = lane; i < padto; i += 64) {
		int cs = 0;
		if (i < dim) {
			const float v = normalize ? mul_nc(xval(x, i), sc) : xval(x, i);
			float c = rintf(__fdiv_rn(sub_nc(v, lo), s));
			c = c >= 0.0f ? c : 0.0f;  // (a NaN element codes as 0)
			c = c <= 255.0f ? c : 255.0f;
			const int ci = (int)c;
			s1 += ci - 128;
			s2 += (long long)(ci - 128) * (ci - 128);
			cs = ci - shift;
		}
		o[i] = (uint8_t)cs;
	}
	if (rt) {
		s1 = wave_sum_i32(s1);
		// (S2 <= 4096 x 2^14 per 64 lanes: the int sum cannot overflow 2^31 below dim = 2^17)
		const int s2w = wave_sum_i32((int)s2);
		if (lane == 0) {
			const float a = mul_nc((float)dim, mul_nc(mid, mid));
			const float b = mul_nc(mul_nc(mul_nc(2.0f, mid), s), (float)s1);
			const float c = mul_nc(mul_nc(s, s), (float)s2w);
			rt[p] = add_nc(add_nc(a, b), c);
		}
	}
}

void launch_sq_encode(const void *X, int xbf16, int ld, int dim, const float *rowaux_f, int normalize,
                      const uint32_t *lslot, int64_t npos, float lo, float s, float mid, int shift, int ldo, int padto,
                      uint8_t *out, float *rt, hipStream_t st) {
	if (npos <= 0) return;
	const dim3 grid((unsigned)((npos + 3) / 4));
	if (xbf16)
		sq_encode_kernel<uint16_t><<<grid, 256, 0, st>>>(static_cast<const uint16_t *>(X), ld, dim, rowaux_f, normalize,
		                                                  lslot, npos, lo, s, mid, shift, ldo, padto, out, rt);
	else
		sq_encode_kernel<float><<<grid, 256, 0, st>>>(static_cast<const float *>(X), ld, dim, rowaux_f, normalize, lslot,
		                                               npos, lo, s, mid, shift, ldo, padto, out, rt);
}

// ---------------------------------------------------------------------------
// search: int8 queries
// ---------------------------------------------------------------------------
// Per query (a workgroup): sq = max|qp| / 127 (0 for a zero query), qi =
// rint(qp / sq) as int8 into Qi [q][ldc] (0 for the padding), par[q] = (sq s,
// (sq mid) f32(sum qi)).  A query with a non-finite element gets zero codes and
// NaN parameters: its keys are NaN, the other queries are untouched.
__global__ __launch_bounds__(256) void sq_query_prep_kernel(const float *__restrict__ Qp, int qld, int dim, int ldc,
                                                            float s, float mid, int8_t *__restrict__ Qi,
                                                            float2 *__restrict__ par) {
	__shared__ float smax[4];
	__shared__ int ssum[4], sbad[4];
	const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
	const float *x = Qp + (int64_t)q * qld;
	float amax = 0.0f;
	int bad = 0;
	for (int i = t; i < dim; i += 256) {
		const float a = fabsf(x[i]);
		if (!(a <= F_MAX)) bad = 1;  // NaN or inf
		else amax = fmaxf(amax, a);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		amax = fmaxf(amax, __shfl_xor(amax, o, 64));
		bad |= __shfl_xor(bad, o, 64);
	}
	if (lane == 0) {
		smax[w] = amax;
		sbad[w] = bad;
	}
	__syncthreads();
	amax = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
	bad = sbad[0] | sbad[1] | sbad[2] | sbad[3];
	const float sq = __fdiv_rn(amax, 127.0f);
	int sum = 0;
	for (int i = t; i < ldc; i += 256) {
		int qi = 0;
		if (i < dim && sq > 0.0f && !bad) {
			float v = rintf(__fdiv_rn(x[i], sq));
			v = v < -127.0f ? -127.0f : (v > 127.0f ? 127.0f : v);
			qi = (int)v;
		}
		sum += qi;
		Qi[(int64_t)q * ldc + i] = (int8_t)qi;
	}
	sum = wave_sum_i32(sum);
	if (lane == 0) ssum[w] = sum;
	__syncthreads();
	if (t == 0) {
		const int tot = ssum[0] + ssum[1] + ssum[2] + ssum[3];
		const float nanv = __builtin_nanf("");
		par[q] = bad ? make_float2(nanv, nanv) : make_float2(mul_nc(sq, s), mul_nc(mul_nc(sq, mid), (float)tot));
	}
}

void launch_sq_query_prep(const float *Qp, int qld, int nq, int dim, int ldc, float s, float mid, int8_t *Qi,
                          float2 *par, hipStream_t st) {
	if (nq <= 0) return;
	sq_query_prep_kernel<<<dim3((unsigned)nq), 256, 0, st>>>(Qp, qld, dim, ldc, s, mid, Qi, par);
}

// ---------------------------------------------------------------------------
// list scan
// ---------------------------------------------------------------------------
// A workgroup takes one IVF_FLAT-style block (256 list positions) and walks its
// list's probing queries in groups of SQ_G: the group's int8 queries sit in LDS,
// the block's codes go HBM -> VGPRs in the MFMA A-operand layout (lane (row r,
// k-group g) holds the 16 bytes k = 16 g .. 16 g + 15 of a 64-deep step; two steps
// in flight), I = sum qi c' by v_mfma_i32_16x16x64_i8 (exact int32), and
//   p = (sq s) f32(I) + (sq mid) f32(sum qi);  key = rt - 2 p (L2) | -p
// in the epilogue.  Per (query, block) each wave sorts its 64 rows' (key, slot)
// words and writes its ko = min(kk, 64) smallest: 4 ko keys, a superset of the
// block's kk smallest, at out [pair][maxb][4 ko].  Dead rows (tombstones, rows
// the predicate leaves out: alpha = +inf in the search's row aux) and padding
// write no key.  4 waves x 64 rows; wave w owns rows 64 w .. 64 w + 63.
template <int METRIC>
__global__ __launch_bounds__(256) void sq_list_scan_kernel(
    const int8_t *__restrict__ lcodes, int ldc, const float *__restrict__ lrt, const float *__restrict__ rowaux_f,
    const int *__restrict__ blk_list, const int64_t *__restrict__ blk_pos0, const int *__restrict__ lblk0,
    const int64_t *__restrict__ loff, const uint32_t *__restrict__ lslot, const int *__restrict__ pstart,
    const int *__restrict__ pairs, int nprobe, int maxb, const int8_t *__restrict__ Qi,
    const float2 *__restrict__ qpar, int ko, uint64_t *__restrict__ out) {
	extern __shared__ __attribute__((aligned(16))) uint8_t sq_smem[];
	const int qrow = ldc + 16;  // padded query row (bytes)
	uint8_t *qs = sq_smem;                                   // [SQ_G][qrow] int8 queries
	uint64_t *sk = reinterpret_cast<uint64_t *>(sq_smem);    // [SQ_G][SQ_KROW] keys (after the K loop)
	__shared__ uint32_t sslot[FLAT_BLK];
	__shared__ float srt[FLAT_BLK];
	__shared__ float2 sqa[SQ_G];
	__shared__ int sq[SQ_G], spair[SQ_G];
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	const int gq = lane >> 4, rr = lane & 15;
	const int b = blockIdx.x;
	const int l = blk_list[b];
	const int pa = pstart[l], pb = pstart[l + 1];
	if (pa >= pb) return;
	const int64_t p0 = blk_pos0[b];
	const int64_t p1 = min<int64_t>(loff[l + 1], p0 + FLAT_BLK);
	const int bi = b - lblk0[l];
	{
		uint32_t s = SLOT_NONE;
		float r = 0.0f;
		if (p0 + t < p1) {
			s = lslot[p0 + t];
			if (s != SLOT_NONE && rowaux_f[raix(s, 0)] == F_INF) s = SLOT_NONE;
			if (METRIC == METRIC_L2) r = lrt[p0 + t];
		}
		sslot[t] = s;
		srt[t] = r;
	}
	const int nw = ldc / 64;
	// this lane's 4 rows: the block is one contiguous 256 x ldc piece of lcodes
	// (positions past the list end read the next list's rows or the zero rows
	// behind the last list; their keys are dropped through sslot)
	const int8_t *xp[4];
#pragma unroll
	for (int rb = 0; rb < 4; ++rb) xp[rb] = lcodes + (p0 + 64 * w + 16 * rb + rr) * (int64_t)ldc + 16 * gq;
	const int KO = 4 * ko;
	for (int g0 = pa; g0 < pb; g0 += SQ_G) {
		const int ng = min(SQ_G, pb - g0);
		__syncthreads();  // (the previous group's key reads done)
		if (t < SQ_G) {
			const int pid = t < ng ? pairs[g0 + t] : -1;
			spair[t] = pid;
			sq[t] = pid < 0 ? -1 : pid / nprobe;
			sqa[t] = pid < 0 ? make_float2(0.f, 0.f) : qpar[pid / nprobe];
		}
		__syncthreads();
		for (int e = t; e < SQ_G * (ldc / 16); e += 256) {
			const int c = e / (ldc / 16), k16 = e % (ldc / 16);
			i32x4 v = {0, 0, 0, 0};
			if (sq[c] >= 0) v = *reinterpret_cast<const i32x4 *>(Qi + (int64_t)sq[c] * ldc + 16 * k16);
			*reinterpret_cast<i32x4 *>(qs + c * qrow + 16 * k16) = v;
		}
		__syncthreads();
		i32x4 acc[4];
#pragma unroll
		for (int rb = 0; rb < 4; ++rb) acc[rb] = i32x4{0, 0, 0, 0};
		const uint8_t *qb = qs + rr * qrow + 16 * gq;
		i32x4 xa[2][4];
		auto ldx = [&](i32x4 (&d)[4], int kw) __attribute__((always_inline)) {
#pragma unroll
			for (int rb = 0; rb < 4; ++rb) d[rb] = *reinterpret_cast<const i32x4 *>(xp[rb] + 64 * kw);
		};
		ldx(xa[0], 0);
		if (nw > 1) ldx(xa[1], 1);
		for (int kw = 0; kw < nw; kw += 2) {
#pragma unroll
			for (int h = 0; h < 2; ++h) {
				const int k = kw + h;
				if (k < nw) {
					const i32x4 bq = *reinterpret_cast<const i32x4 *>(qb + 64 * k);
#pragma unroll
					for (int rb = 0; rb < 4; ++rb)
						acc[rb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(xa[h][rb], bq, acc[rb], 0, 0, 0);
					// refill after the MFMAs that read the registers
					if (k + 2 < nw) ldx(xa[h], k + 2);
				}
			}
		}
		mfma_operand_guard();
		__syncthreads();  // (every wave's query reads done: the keys overwrite them)
		{
			const float2 qa = sqa[rr];
#pragma unroll
			for (int rb = 0; rb < 4; ++rb)
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					const int r = 64 * w + 16 * rb + 4 * gq + i;
					const uint32_t s = sslot[r];
					const float p = add_nc(mul_nc(qa.x, (float)acc[rb][i]), qa.y);
					float key = METRIC == METRIC_L2 ? sub_nc(srt[r], mul_nc(2.0f, p)) : -p;
					key = add_nc(key, 0.0f);  // canonical +0
					sk[rr * SQ_KROW + r] = s != SLOT_NONE ? key64(key, s) : SQ_KEY_NONE;
				}
		}
		__syncthreads();
		// wave w sorts queries w, w + 4, ...: four 64-row runs each
		for (int c = w; c < ng; c += 4) {
			uint64_t *o = out + ((int64_t)spair[c] * maxb + bi) * KO;
#pragma unroll
			for (int ww = 0; ww < 4; ++ww) {
				const uint64_t ks = wave_sort64(sk[c * SQ_KROW + 64 * ww + lane]);
				if (lane < ko) o[ww * ko + lane] = ks;
			}
		}
	}
}

size_t sq_scan_lds_bytes(int ldc) {
	return std::max<size_t>((size_t)SQ_G * (ldc + 16), (size_t)SQ_G * SQ_KROW * sizeof(uint64_t));
}

void launch_sq_list_scan(int metric, const int8_t *lcodes, int ldc, const float *lrt, const float4 *rowaux,
                         const int *blk_list, const int64_t *blk_pos0, const int *lblk0, const int64_t *loff,
                         const uint32_t *lslot, int nblk, const int *pstart, const int *pairs, int nprobe, int maxb,
                         const int8_t *Qi, const float2 *qpar, int ko, uint64_t *out, hipStream_t st) {
	if (nblk <= 0) return;
	if (ldc % 64 || ko < 1 || ko > 64) throw std::runtime_error("IVF_SQ list scan: bad code stride or key count");
	const size_t lds = sq_scan_lds_bytes(ldc);
	const float *ra = reinterpret_cast<const float *>(rowaux);
	auto go = [&](auto kern) {
		HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
		                           (int)lds));
		kern<<<dim3((unsigned)nblk), 256, lds, st>>>(lcodes, ldc, lrt, ra, blk_list, blk_pos0, lblk0, loff, lslot, pstart,
		                                             pairs, nprobe, maxb, Qi, qpar, ko, out);
	};
	switch (metric) {
	case METRIC_L2: go(sq_list_scan_kernel<METRIC_L2>); break;
	case METRIC_DOT: go(sq_list_scan_kernel<METRIC_DOT>); break;
	default: go(sq_list_scan_kernel<METRIC_COSINE>); break;
	}
}

}  // namespace lhip
