// svg_cell_umi.h -- the UMI code of svg_cell_count.hip: three bits a base with A < C < G < N < T, the
// first base most significant (42 bits for SVG_CELL_MAX_UMI bases), so that an unsigned compare of
// codes is memcmp of the texts (the comparator of cell-counts.c:3725-3754) and the Hamming distance
// (cellCounts_hamming_max2_fixlen, :3511) is an XOR, an OR-fold of each 3-bit group and a popcount.
// Plain C as well: the CPU tests check this file through tests/native/cellumi_model.c.
#ifndef SVG_CELL_UMI_H
#define SVG_CELL_UMI_H
#include <stdint.h>

#ifdef __HIPCC__
#define UMI_FN __host__ __device__ static inline
#else
#define UMI_FN static inline
#endif

// A 0, C 1, G 2, N 3, T 4; -1: no UMI character
UMI_FN int umi_char_code(char ch)
{
	switch (ch) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'N': return 3; case 'T': return 4; }
	return -1;
}

// the code of a text of L characters; -1 (all ones) where one is no UMI character
UMI_FN uint64_t umi_encode(const char *text, int L)
{
	uint64_t code = 0;
	for (int k = 0; k < L; k++) {
		const int v = umi_char_code(text[k]);
		if (v < 0) return ~0ull;
		code = code << 3 | (uint64_t)v;
	}
	return code;
}

UMI_FN void umi_decode(uint64_t code, int L, char *out)
{
	for (int k = 0; k < L; k++) out[k] = "ACGNT???"[(code >> (3 * (L - 1 - k))) & 7u];
}

// a packed base (base2int: A 0, G 1, C 2, T 3) and its exception bit (N) as a code character
UMI_FN uint32_t umi_packed_code(uint32_t base, uint32_t exception) { return exception ? 3u : (0x4120u >> (4u * base)) & 15u; }

UMI_FN int umi_hamming(uint64_t a, uint64_t b)
{
	const uint64_t x = a ^ b, y = (x | (x >> 1) | (x >> 2)) & 0x249249249249249ull;
#ifdef __HIP_DEVICE_COMPILE__
	return __popcll(y);
#else
	return __builtin_popcountll(y);
#endif
}

// the two half keys of cell-counts.c:3570 as masks over a code of L bases: characters 0 .. L/2-1 and L/2 .. 2(L/2)-1
UMI_FN uint64_t umi_half_mask(int L, int second)
{
	const int half = L / 2;
	if (!half) return 0;
	return ((1ull << (3 * half)) - 1) << (3 * (L - (second ? 2 : 1) * half));
}
#endif
