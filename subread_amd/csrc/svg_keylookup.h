// svg_keylookup.h -- the equal-key run of one subread key in one index block: the per-key device
// function of svg_probe_keys (svg_keys.hip, which describes the three paths) and of the probe
// kernel of svg_cell_vote_batch (svg_cell.hip).
#ifndef SVG_KEYLOOKUP_H
#define SVG_KEYLOOKUP_H
#include "svg_device.h"

struct KeyTable {
	DevIndex ix;
	const uint32_t *bstart;
	const int16_t *keys;
	uint32_t nb;
};

static inline KeyTable key_table(const svg_index *bk)
{
	KeyTable kt;
	kt.ix = bk->dix;
	kt.bstart = bk->dix.bstart;
	kt.keys = bk->dix.keys;
	kt.nb = bk->dix.nb;
	return kt;
}

// prefill_votes's search, literally (cell-counts.c:432-491)
__device__ __forceinline__ void keys_literal(const KeyTable &kp, uint32_t sub, uint32_t b, uint32_t &f, uint32_t &c)
{
	{
		const uint32_t base = kp.bstart[b];
		const int items = (int)(kp.bstart[b + 1] - base);
		const int16_t *ck = kp.keys + base;
		const int16_t key = (int16_t)(sub / kp.nb);
		f = 0;
		c = 0;
		if (items > 0) {
			int imin = 0, imax = items - 1, last;
			bool found = true;
			for (;;) {
				last = (imin + imax) / 2;
				const int16_t cur = ck[last];
				if (cur > key) imax = last - 1;
				else if (cur < key) imin = last + 1;
				else break;
				if (imax < imin) { found = false; break; }
			}
			if (found) {
				imax -= imin;
				const int start = last;
				int stoploc;
				for (int step = imax / 4; step > 1; step /= 3)
					for (;;) {
						const int tl = last + step;
						if (tl >= items || ck[tl] != key) break;
						last = tl;
					}
				for (;;) {
					last++;
					if (last == items || ck[last] != key) { stoploc = last; last = start; break; }
				}
				for (int step = imax / 4; step > 1; step /= 3)
					for (;;) {
						const int tl = last - step;
						if (tl < imin || ck[tl] != key) break;
						last = tl;
					}
				while (!(last == imin || ck[last - 1] != key)) last--;
				f = (uint32_t)last;
				c = (uint32_t)(stoploc - last);
			}
		}
	}
}

#define KEYS_LITERAL 0
#define KEYS_CODE    1
#define KEYS_KHASH   2

// the image a block's lookups take (option keys_literal forces the literal search)
static inline int key_image(const svg_index *bk)
{
	const bool lit = svg_get_option("keys_literal") != 0;
	if (!lit && bk->dix.bcode) return KEYS_CODE;
	if (!lit && bk->dix.khash && bk->dix.ksorted) return KEYS_KHASH;
	return KEYS_LITERAL;
}

// key sub's run in its bucket b (returned): f = bucket-local index of its first item, c = its
// length (0: absent, f = 0)
template <int IMG>
__device__ __forceinline__ uint32_t key_run(const KeyTable &kp, uint32_t sub, uint32_t &f, uint32_t &c)
{
	const uint32_t q = sub / kp.nb, b = sub - q * kp.nb;
	f = 0;
	c = 0;
	bool literal = IMG == KEYS_LITERAL;
	if (IMG == KEYS_CODE) {
		// the bucket's 32-byte code: the run of key_hi = q is [fe, ee) of the bucket's items
		const uint4 *c4 = kp.ix.bcode + 2 * (size_t)b;
		const uint4 u0 = c4[0], u1 = c4[1];
		const uint32_t n = u0.y & 255u;
		literal = n == 255u;
		if (!literal && n) {
			const uint64_t z[4] = {~(((uint64_t)u0.y << 32) | u0.x) & ~0xffffffffffull, ~(((uint64_t)u0.w << 32) | u0.z),
			                       ~(((uint64_t)u1.y << 32) | u1.x), ~(((uint64_t)u1.w << 32) | u1.z)};
			const int k = (int)q;
			const int fe = k ? code_zero(z, k - 1) - 40 - (k - 1) : 0;
			const int ee = code_zero(z, k) - 40 - k;
			if (ee > fe) { f = (uint32_t)fe; c = (uint32_t)(ee - fe); }
		}
	} else if (IMG == KEYS_KHASH) {
		// (the image keys a run by (u16)key_hi * nb + bucket: quotients past 16 bits, which only
		// tiny indexes have, compare as wrapped shorts in the reference -- literal search)
		literal = q > 0xffffu || !((kp.ix.ksorted[b >> 5] >> (b & 31u)) & 1u);
		if (!literal) {
			uint2 rec;
			if (khash_find(kp.ix, sub, rec)) {
				{
					const uint32_t fwd = rec.y & 0xffffu, bwd = rec.y >> 16;
					f = rec.x - bwd - kp.bstart[b];
					c = fwd + bwd;
				}
			}
		}
	}
	if (literal) keys_literal(kp, sub, b, f, c);
	return b;
}

#endif
