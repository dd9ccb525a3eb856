// Predicate programs of filtered search: the flat postfix form a Lance-SQL
// predicate compiles to (meta.cpp compile_predicate) and its per-row
// interpreter, shared by the host (lance_hip_predicate_mask_program) and the
// device evaluator (filter_kernels.hip).  The interpreter reproduces the
// vectorised host evaluator (meta.cpp Eval) value for value: SQL three-valued
// logic, exact int64 compares, (double) of an integer against a float, NaN as
// the largest value and equal to NaN.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lhip {

// Limits of a device-evaluable program (a predicate past any of them is
// evaluated by the host evaluator instead).  The value stack is two 64-bit
// words (TRUE bits, NULL bits), so the interpreter needs no per-thread array.
constexpr int FP_MAX_INSTR = 256;
constexpr int FP_MAX_LITS = 4096;
constexpr int FP_MAX_COLS = 16;
constexpr int FP_MAX_STACK = 64;

enum FpOp : uint8_t {
	FP_CONST = 0,   // push a constant: a = 0 FALSE, 1 TRUE, 2 NULL
	FP_CMP_CL,      // push col[a] <cmp> lit[b]      (ta: column class, tb: literal class)
	FP_CMP_CC,      // push col[a] <cmp> col[b]      (ta, tb: column classes)
	FP_ISNULL_COL,  // push col[a] IS [NOT] NULL     (tb & 1: NOT)
	FP_BOOLCOL,     // push the boolean column a
	FP_IN_CL,       // push col[a] [NOT] IN (lit[b] .. lit[b + n))  (ta: column class, cmp: the literals' class,
	                //                                               tb & 1: NOT, tb & 2: the list has a NULL)
	FP_AND,         // pop b, a; push a AND b
	FP_OR,          // pop b, a; push a OR b
	FP_NOT,         // top = NOT top
	FP_ISNULL,      // top = top IS [NOT] NULL       (tb & 1: NOT)
};
enum FpCmp : uint8_t { FP_EQ = 0, FP_NE, FP_LT, FP_LE, FP_GT, FP_GE };
// number class of an operand: int64 (integers, booleans as 0 / 1) or f64.  Two
// int64 operands compare exactly; any other pair compares as doubles.
enum FpClass : uint8_t { FP_INT = 0, FP_FLT = 1 };

struct FpInstr {
	uint8_t op, cmp, ta, tb;
	uint16_t a, b;
	uint32_t n;
};

// one referenced column: 8-byte values per slot (int64 or f64 bits) and the
// validity bytes (null: the column has no NULLs, i.e. `label`)
struct FpCol {
	const void *vals;
	const uint8_t *valid;
};

__host__ __device__ inline uint64_t fp_load(const void *p, int64_t i) {
	uint64_t u;
	__builtin_memcpy(&u, static_cast<const char *>(p) + i * 8, 8);
	return u;
}
__host__ __device__ inline double fp_as_double(uint64_t u, int cls) {
	if (cls == FP_INT) return (double)(int64_t)u;
	double d;
	__builtin_memcpy(&d, &u, 8);
	return d;
}
// sign of x - y in the evaluator's order
__host__ __device__ inline int fp_cmp3(uint64_t x, int cx, uint64_t y, int cy) {
	if (cx == FP_INT && cy == FP_INT) {
		const int64_t a = (int64_t)x, b = (int64_t)y;
		return (a > b) - (a < b);
	}
	const double a = fp_as_double(x, cx), b = fp_as_double(y, cy);
	const bool na = a != a, nb = b != b;
	if (na || nb) return na && nb ? 0 : (na ? 1 : -1);
	return (a > b) - (a < b);
}
__host__ __device__ inline bool fp_test(int c, int op) {
	switch (op) {
	case FP_EQ: return c == 0;
	case FP_NE: return c != 0;
	case FP_LT: return c < 0;
	case FP_LE: return c <= 0;
	case FP_GT: return c > 0;
	default: return c >= 0;
	}
}

// Runs the program for slot r; true iff the predicate is TRUE (NULL is not).
__host__ __device__ inline bool fp_eval_row(const FpInstr *code, int n_code, const uint64_t *lits, const FpCol *cols,
                                            int64_t r) {
	uint64_t sv = 0, sn = 0;  // stack, top at bit 0: TRUE bits and NULL bits (never both)
	for (int pc = 0; pc < n_code; ++pc) {
		const FpInstr in = code[pc];
		uint64_t v = 0, nl = 0;
		switch (in.op) {
		case FP_CONST:
			v = in.a == 1;
			nl = in.a == 2;
			break;
		case FP_CMP_CL: {
			const FpCol c = cols[in.a];
			if (c.valid && !c.valid[r]) nl = 1;
			else v = fp_test(fp_cmp3(fp_load(c.vals, r), in.ta, lits[in.b], in.tb), in.cmp);
			break;
		}
		case FP_CMP_CC: {
			const FpCol c = cols[in.a], d = cols[in.b];
			if ((c.valid && !c.valid[r]) || (d.valid && !d.valid[r])) nl = 1;
			else v = fp_test(fp_cmp3(fp_load(c.vals, r), in.ta, fp_load(d.vals, r), in.tb), in.cmp);
			break;
		}
		case FP_ISNULL_COL: {
			const FpCol c = cols[in.a];
			const bool isnull = c.valid && !c.valid[r];
			v = isnull != (bool)(in.tb & 1);
			break;
		}
		case FP_BOOLCOL: {
			const FpCol c = cols[in.a];
			if (c.valid && !c.valid[r]) nl = 1;
			else v = fp_load(c.vals, r) != 0;
			break;
		}
		case FP_IN_CL: {
			const FpCol c = cols[in.a];
			if (c.valid && !c.valid[r]) {
				nl = 1;
			} else {
				const uint64_t x = fp_load(c.vals, r);
				bool hit = false;
				for (uint32_t i = 0; i < in.n; ++i) hit |= fp_cmp3(x, in.ta, lits[in.b + i], in.cmp) == 0;
				if (hit) v = 1;
				else if (in.tb & 2) nl = 1;
				if ((in.tb & 1) && !nl) v ^= 1;
			}
			break;
		}
		case FP_AND:
		case FP_OR: {
			const uint64_t bv = sv & 1, bn = sn & 1, av = (sv >> 1) & 1, an = (sn >> 1) & 1;
			sv >>= 2;
			sn >>= 2;
			if (in.op == FP_AND) {
				const uint64_t f = ((an | av) ^ 1) | ((bn | bv) ^ 1);  // either side FALSE
				v = av & bv;
				nl = (an | bn) & (f ^ 1);
			} else {
				v = av | bv;
				nl = (an | bn) & (v ^ 1);
			}
			break;
		}
		case FP_NOT:
			v = ((sv | sn) & 1) ^ 1;
			nl = sn & 1;
			sv >>= 1;
			sn >>= 1;
			break;
		default:  // FP_ISNULL
			v = (sn & 1) ^ (uint64_t)(in.tb & 1);
			sv >>= 1;
			sn >>= 1;
			break;
		}
		sv = (sv << 1) | v;
		sn = (sn << 1) | nl;
	}
	return sv & 1;
}

}  // namespace lhip
