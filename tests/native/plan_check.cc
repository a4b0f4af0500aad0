// plan_check.cc -- svg_plan.h against the literal arithmetic it replaces (host only):
//   * per read: step and number of probes, per probe: the read offset, for every length
//     0..SVG_READ_KEEP (and past it: the clamp), total_subreads 10 and 14, every gap 1..192
//     (the index builder makes 1 and 3; a loaded index may carry any, and a gap above 192 has no
//     probe inside the 192-probe bound) and every probe below the 192-probe bound;
//   * the multiply-shift quotients against '/', the packed plan against what went into it;
//   * the slot-major probe index of a read group against the division form, per_read 2..768,
//     1..64 reads present.
// Prints the number of comparisons and exits 0, or the first difference and exits 1.
#include <stdio.h>
#include <stdint.h>
#include <vector>
#include "svg_plan.h"

static long long checks = 0;

// probe_key as it stood before the plan: false when the read has no probe p
static bool literal_off(int len, int gap, int total_subreads, int p, int *step_out, int *np_out, int *off_out)
{
	if (len > SVG_READ_KEEP) len = SVG_READ_KEEP;
	if (len < 15 + gap) return false;
	const int cr = (len - 15 - gap) << 16;
	int step;
	if (len <= 160) { step = cr / (total_subreads - 1); if (step < (gap << 16)) step = gap << 16; }
	else { step = 6 << 16; if (cr / step > 62) step = cr / 62; }
	const int np = (1 + cr / step) * gap;
	*step_out = step;
	*np_out = np;
	if (p >= np) return false;
	const int k = p / gap, x = p - k * gap;
	int off = (int)(((int64_t)step * k) >> 16);
	if (gap > 1) off -= off % gap - x;
	*off_out = off;
	return true;
}

static int check_plan(void)
{
	const int subs[2] = {10, 14};
	for (int gap = 1; gap <= 192; gap++) {
		const uint32_t magic = svg_plan_gap_magic(gap);
		if (gap > 1) for (uint32_t x = 0; x <= 4096; x++) {
			checks++;
			if (svg_plan_div_gap(x, magic) != x / (uint32_t)gap) { printf("div: x %u gap %d\n", x, gap); return 1; }
		}
		for (int si = 0; si < 2; si++) for (int len = 0; len <= SVG_READ_KEEP + 2; len++) {
			int clen, step;
			const int np = svg_plan_read(len, gap, subs[si], &clen, &step);
			if (clen != (len > SVG_READ_KEEP ? SVG_READ_KEEP : len)) { printf("clen: len %d\n", len); return 1; }
			// the packed plan gives back base, length and step, and its clamped probe count
			// compares like np with every probe number below the bound
			uint32_t w[3];
			const uint64_t base = 0xfedcba987654ull - (uint64_t)len * 977u;
			svg_plan_pack(base, clen, step, np, w);
			if (svg_plan_base(w) != base || svg_plan_len(w) != clen || svg_plan_step(w) != step ||
			    svg_plan_np(w) != (np > 255 ? 255 : np)) { printf("pack: len %d gap %d n %d\n", len, gap, subs[si]); return 1; }
			for (int p = 0; p < 192; p++) {
				int lstep = 0, lnp = 0, loff = 0;
				const bool has = literal_off(len, gap, subs[si], p, &lstep, &lnp, &loff);
				checks++;
				if (has != (p < np)) { printf("has: len %d gap %d n %d p %d: %d, plan np %d\n", len, gap, subs[si], p, (int)has, np); return 1; }
				if (np && (step != lstep || np != lnp)) { printf("step/np: len %d gap %d n %d: %d %d, literal %d %d\n", len, gap, subs[si], step, np, lstep, lnp); return 1; }
				if (has && svg_plan_off(step, p, gap, magic) != loff) {
					printf("off: len %d gap %d n %d p %d: %d, literal %d\n", len, gap, subs[si], p, svg_plan_off(step, p, gap, magic), loff);
					return 1;
				}
			}
		}
	}
	return 0;
}

template <int ENDS>
static int check_index(void)
{
	for (uint32_t per_read = 2 * ENDS; per_read <= 768; per_read += 2 * ENDS) {
		const uint32_t nps = per_read / (2 * ENDS), lg = svg_plan_group_log2(2048, per_read), G = 1u << lg;
		// the group: the largest power of two <= min(64, 2048 / per_read)
		if (G > 64 || G * per_read > 2048 || (G < 64 && 2 * G * per_read <= 2048)) { printf("group: per_read %u G %u\n", per_read, G); return 1; }
		for (uint32_t nr = 1; nr <= G; nr++) {
			std::vector<char> seen((size_t)nr * per_read, 0);
			for (uint32_t i = 0; i < per_read * G; i++) {
				uint32_t rl, slot;
				int e, s, p;
				svg_plan_index<ENDS>(i, lg, nps, &rl, &slot, &e, &s, &p);
				checks++;
				if (i != slot * G + rl || rl >= G || slot >= per_read) { printf("split: i %u\n", i); return 1; }
				if (rl >= nr) continue;   // idle lane of a partial group
				// the division form, on the read-major index of the same probe
				const uint32_t j = rl * per_read + slot;
				const uint32_t drl = j / per_read, rem = j - drl * per_read;
				const int de = ENDS == 2 ? (int)(rem / (2 * nps)) : 0;
				const uint32_t rem2 = rem - (uint32_t)de * 2 * nps;
				const int ds = rem2 >= nps ? 1 : 0;
				const int dp = (int)(rem2 - (uint32_t)ds * nps);
				if (drl != rl || rem != slot || de != e || ds != s || dp != p) {
					printf("index: ENDS %d per_read %u nr %u i %u: (%u %u %d %d %d), division (%u %u %d %d %d)\n", ENDS, per_read, nr, i,
					       rl, slot, e, s, p, drl, rem, de, ds, dp);
					return 1;
				}
				if (seen[j]++) { printf("index: probe %u twice\n", j); return 1; }
			}
			for (size_t j = 0; j < seen.size(); j++) if (!seen[j]) { printf("index: probe %zu missing\n", j); return 1; }
		}
	}
	return 0;
}

int main(void)
{
	if (check_plan() || check_index<1>() || check_index<2>()) return 1;
	printf("ok %lld\n", checks);
	return 0;
}
