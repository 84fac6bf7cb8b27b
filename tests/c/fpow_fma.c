/* The one operation of docs/SPEC.md §19 that numpy cannot make: p = fma(re, re, im*im) in float32, with a real fused
 * multiply-add (a float64 emulation double-rounds in rare cases).  tests/fpow_ref.py compiles this into a small shared object
 * and calls it through ctypes. */
#include <math.h>
#include <stddef.h>

void fpow_p(const float *re, const float *im, float *out, size_t n)
{
    size_t i;
    for (i = 0; i < n; i++)
    {
        const volatile float sq = im[i] * im[i]; /* rounded to float32 before the fused operation */
        out[i] = fmaf(re[i], re[i], sq);
    }
}
