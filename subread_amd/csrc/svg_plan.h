// svg_plan.h -- the per-read arithmetic of the subread probes (core.c:3117-3171), in one place for
// the probe kernels, the host and the host test (tests/native/plan_check.cc): what depends on the
// read alone (clamped length, subread step, number of probes), the per-probe offset without a
// division, and the slot-major probe index of probe_line_kernel's read groups.
#ifndef SVG_PLAN_H
#define SVG_PLAN_H
#include <stdint.h>
#include "subread_vote.h"

#if defined(__HIPCC__)
#define SVG_PLAN_FN __host__ __device__ __forceinline__
#else
#define SVG_PLAN_FN static inline
#endif

// probes of one strand of a read of len bases: 0 if it has none (shorter than 15 + gap), else
// applied subreads x gap; *clen = the length read_line keeps, *step = the subread step (16.16)
SVG_PLAN_FN int svg_plan_read(int len, int gap, int total_subreads, int *clen, int *step)
{
	if (len > SVG_READ_KEEP) len = SVG_READ_KEEP;
	*clen = len;
	*step = 0;
	if (len < 15 + gap) return 0;
	const int cr = (len - 15 - gap) << 16;
	int st;
	if (len <= 160) { st = cr / (total_subreads - 1); if (st < (gap << 16)) st = gap << 16; }
	else { st = 6 << 16; if (cr / st > 62) st = cr / 62; }
	*step = st;
	return (1 + cr / st) * gap;
}

// x / gap as a multiply-shift: exact for gap >= 2 and x * gap < 2^32 (every probe number below
// the 192-probe bound and every read offset); gap 1 needs no quotient and has no 32-bit constant
SVG_PLAN_FN uint32_t svg_plan_gap_magic(int gap) { return gap > 1 ? 0xffffffffu / (uint32_t)gap + 1u : 0u; }
SVG_PLAN_FN uint32_t svg_plan_div_gap(uint32_t x, uint32_t magic) { return (uint32_t)(((uint64_t)x * magic) >> 32); }

// read offset of probe p (subread p / gap, gap slot p % gap) of a read with subread step `step`
SVG_PLAN_FN int svg_plan_off(int step, int p, int gap, uint32_t magic)
{
	if (gap == 1) return (int)(uint32_t)(((uint64_t)(uint32_t)step * (uint32_t)p) >> 16);
	const uint32_t k = svg_plan_div_gap((uint32_t)p, magic), x = (uint32_t)p - k * (uint32_t)gap;
	const uint32_t off = (uint32_t)(((uint64_t)(uint32_t)step * k) >> 16);
	return (int)(off - (off - svg_plan_div_gap(off, magic) * (uint32_t)gap) + x);
}

// a read end's plan in three words (probe_line_kernel keeps it in LDS and in registers): the
// read's base (below 2^48: an offset into one buffer), kept length (<= SVG_READ_KEEP < 2^16),
// subread step (below 2^24 for every gap below 256: at most (len - 16) << 16 / 62, 144 << 16 or
// gap << 16) and number of probes, clamped to 255 -- a probe number stays below the 192-probe
// bound, so the comparison with it is unchanged.  An index with a gap above 192 is only voted on
// with reads that have no probe within the bound (one probe slot, p = 0, offset 0 whatever the
// step), so the cut of a wider step changes nothing either.
SVG_PLAN_FN void svg_plan_pack(uint64_t base, int len, int step, int np, uint32_t w[3])
{
	w[0] = (uint32_t)base;
	w[1] = ((uint32_t)(base >> 32) & 0xffffu) | ((uint32_t)len << 16);
	w[2] = ((uint32_t)step & 0xffffffu) | ((uint32_t)(np > 255 ? 255 : np) << 24);
}
SVG_PLAN_FN uint64_t svg_plan_base(const uint32_t w[3]) { return w[0] | ((uint64_t)(w[1] & 0xffffu) << 32); }
SVG_PLAN_FN int svg_plan_len(const uint32_t w[3]) { return (int)(w[1] >> 16); }
SVG_PLAN_FN int svg_plan_step(const uint32_t w[3]) { return (int)(w[2] & 0xffffffu); }
SVG_PLAN_FN int svg_plan_np(const uint32_t w[3]) { return (int)(w[2] >> 24); }

// reads per group of probe_line_kernel: the largest power of two <= min(64, recs / per_read)
// (at least 1), as its log2
SVG_PLAN_FN uint32_t svg_plan_group_log2(uint32_t recs, uint32_t per_read)
{
	uint32_t g = recs / per_read, lg = 0;
	if (g > 64u) g = 64u;
	while ((2u << lg) <= g) lg++;
	return lg;
}

// probe i of a group of 1 << lg reads, slot-major (i = slot * G + read): the read within the
// group, and the slot = (end * 2 + strand) * nps + p split without a division
template <int ENDS>
SVG_PLAN_FN void svg_plan_index(uint32_t i, uint32_t lg, uint32_t nps, uint32_t *rl, uint32_t *slot, int *e, int *s, int *p)
{
	*rl = i & ((1u << lg) - 1u);
	const uint32_t sl = i >> lg;
	uint32_t es = sl >= nps ? 1u : 0u;
	if (ENDS == 2) es += (sl >= 2u * nps ? 1u : 0u) + (sl >= 3u * nps ? 1u : 0u);
	*slot = sl;
	*e = (int)(es >> 1);
	*s = (int)(es & 1u);
	*p = (int)(sl - es * nps);
}

#endif
