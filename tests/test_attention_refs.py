"""CPU: the checkers of tests/test_gpu_attention_core.py -- tests/rng_host.py attn_quad_keep and tests/attention_refs.py.

  1. attn_quad_keep against the product's own `__host__` generator functions (csrc/common.h compiled into a probe program, the way
     tests/test_rng_host.py reaches them) and against a scalar transcription kept next to the cited lines; its keep rate;
  2. for every case the GPU file lists, the operand-rounding model evaluated in fp32 sits inside the bound with F = (N + 64) 2^-24;
  3. every mutant of the reference leaves the bound on at least one listed case of each kernel form it can affect, in both types."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import attention_refs as AR
from tests import rng_host as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DTYPES = ["bf16", "fp16"]
SEED, FWD, SITE = 0x1234ABCD5678, 2, 3
QUAD_PROBE = [(N, p, grow) for N in (5, 132) for p in (0.1, 0.7) for grow in (0, 6)]

PROBE = r'''
#include "common.h"
#include <cstdio>
int main(int argc, char** argv) {
    const unsigned long long seed = %dull;
    const unsigned Ns[2] = {5u, 132u};
    const float ps[2] = {0.1f, 0.7f};
    const unsigned rows[2] = {0u, 6u};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int c = 0; c < 2; ++c)
                for (unsigned h = 0; h < 4; ++h) {
                    const unsigned N = Ns[a];
                    RngKey k = rng_stream_key(rng_row_key((uint32_t)seed, (uint32_t)(seed >> 32), %du, rows[c]), rng_layer_salt(%du));
                    k.k0 = fmix32(k.k0 + (h + 1u) * 0x9E3779B9u);  // unet_kernels.hip attn_drop_key
                    const uint32_t th = keep_threshold8(ps[b]);
                    unsigned acc = 0, kept = 0;
                    for (unsigned i = 0; i < N; ++i)
                        for (unsigned j = 0; j < N; ++j) {
                            const unsigned bit = rng_keep8(i * N + j, k, th) ? 1u : 0u;
                            acc = acc * 31u + bit;
                            kept += bit;
                        }
                    printf("%%u %%d %%u %%u %%u %%u %%u\n", N, b, rows[c], h, th, acc, kept);
                }
    return 0;
}
'''


def _fold(bits):
    acc = 0
    for b in bits.reshape(-1):
        acc = (acc * 31 + int(b)) & 0xFFFFFFFF
    return acc


# ---- scalar transcription (used where no hipcc is at hand, and always at N = 5) ----------------------------------------------------
def _fmix32(h):  # common.h:127 fmix32
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _pair_word(i, k0, k1):  # common.h:166-174 rng_pair_word (mul_u24: the low 24 bits of both factors)
    x = (i * 0x9E3779B1 + k0) & 0xFFFFFFFF
    x ^= x >> 15
    x = ((x & 0xFFFFFF) * 0x735A2D + k1) & 0xFFFFFFFF
    x ^= x >> 13
    x = ((x & 0xFFFFFF) * 0x97E5B5) & 0xFFFFFFFF
    return x ^ (x >> 16)


def _scalar_quad_keep(N, p, seed, fwd, site, grow):
    lo, hi = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    a = _fmix32(lo ^ _fmix32(hi + 0x9E3779B9 * (fwd + 1)))                # common.h:178-182 rng_row_key
    b = _fmix32(a + 0x85EBCA77 * (grow + 1))
    r0, r1 = b, _fmix32(b ^ hi ^ 0x27D4EB2F)
    s0 = _fmix32(0x9E3779B9 * (site + 1))                                  # common.h:185-188 rng_layer_salt
    s1 = _fmix32(s0 + 0x165667B1)
    k0, k1 = r0 ^ s0, (r1 + s1) & 0xFFFFFFFF                               # common.h:190-192 rng_stream_key
    keep32 = np.float32(np.float32(1.0) - np.float32(p)) * np.float32(256.0)  # common.h:206-210 keep_threshold8
    th = max(1, 256 if keep32 >= 256.0 else int(keep32))
    out = np.zeros((4, N, N), dtype=bool)
    for h in range(4):
        kh = _fmix32(k0 + (h + 1) * 0x9E3779B9)                            # unet_kernels.hip:1532-1536 attn_drop_key
        for i in range(N):
            for j in range(N):
                e = (i * N + j) & 0xFFFFFFFF
                out[h, i, j] = ((_pair_word(e >> 2, kh, k1) >> (8 * (e & 3))) & 0xFF) < th  # common.h:220-223 rng_keep8
    return out, th


def test_quad_restatement_equals_the_scalar_transcription():
    for p in (0.1, 0.7):
        for grow in (0, 6):
            got, scale = R.attn_quad_keep(5, p, SEED, FWD, SITE, grow)
            want, th = _scalar_quad_keep(5, p, SEED, FWD, SITE, grow)
            assert np.array_equal(got, want) and scale == 256.0 / th and th == R.keep_threshold8(p), (p, grow)
    assert [R.keep_threshold8(p) for p in (0.0, 0.1, 0.3, 0.7, 0.999)] == [256, 230, 179, 76, 1]


def test_quad_restatement_equals_the_product_host_code(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:  # no compiler: the scalar transcription stands in, at both token counts
        for N, p, grow in QUAD_PROBE:
            assert np.array_equal(R.attn_quad_keep(N, p, SEED, FWD, SITE, grow)[0], _scalar_quad_keep(N, p, SEED, FWD, SITE, grow)[0])
        return
    src, exe = tmp_path / "probe.hip", tmp_path / "probe"
    src.write_text(PROBE % (SEED, FWD, SITE))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "dyffusion_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(lines) == 2 * 2 * 2 * 4
    for line in lines:
        N, pi, grow, h, th, acc, kept = (int(v) for v in line.split())
        p = (0.1, 0.7)[pi]
        keep, scale = R.attn_quad_keep(N, p, SEED, FWD, SITE, grow)
        assert th == R.keep_threshold8(p) and scale == 256.0 / th
        assert int(keep[h].sum()) == kept and _fold(keep[h]) == acc, line


def test_quad_keep_rate_and_the_mutant_restatement():
    for p in (0.1, 0.7):
        rows = np.stack([R.attn_quad_keep(132, p, SEED, FWD, SITE, g)[0] for g in (0, 6)])
        k = R.keep_threshold8(p)
        rate, se = rows.mean(), np.sqrt((k / 256) * (1 - k / 256) / rows.size)
        print(f"quad stream p={p}: keep rate {rate:.5f}, k / 256 = {k / 256:.5f}, standard error {se:.2e}")
        assert abs(rate - k / 256) <= 3 * se
        assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[0][0], rows[0][1])
        assert np.array_equal(AR.quad_keep_row(132, p, SEED, FWD, SITE, 6), rows[1])
        for m in AR.QUAD_MUTANTS:
            assert not np.array_equal(AR.quad_keep_row(132, p, SEED, FWD, SITE, 6, m), rows[1]), m


# ------------------------------------------------------------------------------------------------ 2. the model inside the bound
def _quad_case(N, nb, grow, p, score, dtype, mutant=None):
    keep, scale = AR.quad_keep(nb, N, p, AR.quad_seed(N), grow, mutant)
    return AR.core_inputs(nb, N, score, dtype), keep, scale


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,switch,N", AR.CORE_FORMS, ids=[AR.case_id(*c) for c in AR.CORE_FORMS])
def test_fp32_model_sits_inside_the_bound_dropout_free(form, switch, N, dtype):
    for nb, case in AR.CORE_ROWS:
        qkv = AR.core_inputs(nb, N, case, dtype)
        r = AR.worst_ratio(AR.model_fp32(qkv, dtype, form), AR.reference(qkv, dtype, form), dtype, form, AR.f_cpu(N))
        print(f"{form} N={N} nb={nb} {case} {dtype}: fp32 model at {r:.3f} of the bound")
        assert r <= 1.0, (nb, case, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,switch,N", AR.QUAD_SCORE_FORMS, ids=[AR.case_id(*c) for c in AR.QUAD_SCORE_FORMS])
def test_fp32_model_sits_inside_the_bound_quad_dropout(form, switch, N, dtype):
    for nb, grow, p in AR.QUAD_ROWS:
        for score in AR.QUAD_SCORES:
            qkv, keep, scale = _quad_case(N, nb, grow, p, score, dtype)
            r = AR.worst_ratio(AR.model_fp32(qkv, dtype, form, keep, scale), AR.reference(qkv, dtype, form, keep, scale), dtype, form, AR.f_cpu(N))
            print(f"{form} N={N} nb={nb} p={p} {score} {dtype}: fp32 model at {r:.3f} of the bound")
            assert r <= 1.0, (nb, p, score, r)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,switch,N", AR.MASK_FORMS, ids=[AR.case_id(*c) for c in AR.MASK_FORMS])
def test_fp32_model_sits_inside_the_bound_injected_masks(form, switch, N, dtype):
    qkv = AR.core_inputs(AR.MASK_NB, N, "randn", dtype)
    keep, scale = AR.bernoulli_mask(AR.MASK_NB, N, AR.MASK_P, N), 1.0 / (1.0 - AR.MASK_P)
    r = AR.worst_ratio(AR.model_fp32(qkv, dtype, form, keep, scale), AR.reference(qkv, dtype, form, keep, scale), dtype, form, AR.f_cpu(N))
    print(f"{form} N={N} injected mask {dtype}: fp32 model at {r:.3f} of the bound")
    assert r <= 1.0


# ------------------------------------------------------------------------------------------------ 3. mutants
FORMS = (AR.PLAIN, AR.FA2, AR.FA4_4, AR.FA4_8)


def _f(form, N):  # the looser of the two slacks a test of this pull request uses
    return max(AR.f_cpu(N), AR.F_GPU[AR.family_of(form)])


def _margin(wrong, ref, dtype, form, N):
    return float(((wrong - ref["want"]).abs() / AR.bound(ref, dtype, form, _f(form, N))).max())


def _best(form, cases, run):
    """largest margin of a mutant over the listed cases of one form (smallest token counts first, stops at the first that shows)"""
    best = 0.0
    for f, _, N in sorted(cases, key=lambda c: c[2]):
        if f != form:
            continue
        best = max(best, run(N))
        if best > 1.0:
            break
    return best


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", ["row_reads_previous_v", "no_score_scale", "padded_keys_in_normaliser", "heads_swapped"])
def test_reference_mutants_leave_the_bound_dropout_free(mutant, dtype):
    for form in FORMS:
        def run(N):
            if mutant == "padded_keys_in_normaliser" and N % 64 == 0:
                return 0.0
            worst = 0.0
            for nb, case in AR.CORE_ROWS[:2]:  # nb = 3: small, spread
                qkv = AR.core_inputs(nb, N, case, dtype)
                ref = AR.reference(qkv, dtype, form)
                worst = max(worst, _margin(AR.reference(qkv, dtype, form, mutant=mutant)["want"], ref, dtype, form, N))
            return worst
        m = _best(form, AR.CORE_FORMS, run)
        print(f"{mutant} on {form} ({dtype}): {m:.3g} x the bound")
        assert m > 1.0, (form, m)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", ["normaliser_after_dropout"] + list(AR.QUAD_MUTANTS) + ["scale_1_over_1_minus_p"])
def test_reference_mutants_leave_the_bound_quad_dropout(mutant, dtype):
    for form in FORMS:
        def run(N, rows=AR.QUAD_ROWS[:1]):  # nb = 3 at row offset 5, p = 0.7
            worst = 0.0
            for nb, grow, p in rows:
                qkv, keep, scale = _quad_case(N, nb, grow, p, "randn", dtype)
                ref = AR.reference(qkv, dtype, form, keep, scale)
                if mutant in AR.QUAD_MUTANTS:
                    wrong = AR.reference(qkv, dtype, form, AR.quad_keep(nb, N, p, AR.quad_seed(N), grow, mutant)[0], scale)
                elif mutant == "scale_1_over_1_minus_p":
                    wrong = AR.reference(qkv, dtype, form, keep, 1.0 / (1.0 - p))
                else:
                    wrong = AR.reference(qkv, dtype, form, keep, scale, mutant=mutant)
                worst = max(worst, _margin(wrong["want"], ref, dtype, form, N))
            return worst
        m = _best(form, AR.QUAD_SCORE_FORMS, run)
        print(f"{mutant} on {form} ({dtype}, p = 0.7): {m:.3g} x the bound")
        assert m > 1.0, (form, m)
        if mutant == "scale_1_over_1_minus_p":  # 256 / 230 against 1 / 0.9: 0.17 %, below half an ulp of bf16
            m01 = _best(form, AR.QUAD_SCORE_FORMS, lambda N: run(N, AR.QUAD_ROWS[1:]))
            print(f"    at p = 0.1: {m01:.3g} x the bound" + (" -- invisible here; the survivor values of the GPU file's mask test tell the two apart" if m01 <= 1.0 else ""))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mutant", ["normaliser_after_dropout", "mask_ignores_the_row"])
def test_reference_mutants_leave_the_bound_injected_masks(mutant, dtype):
    scale = 1.0 / (1.0 - AR.MASK_P)
    for form in (AR.FA2, AR.PLAIN):
        def run(N):
            qkv = AR.core_inputs(AR.MASK_NB, N, "randn", dtype)
            keep = AR.bernoulli_mask(AR.MASK_NB, N, AR.MASK_P, N)
            ref = AR.reference(qkv, dtype, form, keep, scale)
            if mutant == "mask_ignores_the_row":  # ((h * N + i) * N + j): every row reads the first row's masks
                wrong = AR.reference(qkv, dtype, form, keep[:1].expand_as(keep), scale)
            else:
                wrong = AR.reference(qkv, dtype, form, keep, scale, mutant=mutant)
            return _margin(wrong["want"], ref, dtype, form, N)
        m = _best(form, AR.MASK_FORMS, run)
        print(f"{mutant} on {form} ({dtype}): {m:.3g} x the bound")
        assert m > 1.0, (form, m)
