"""Host side of tests/test_gpu_stem8.py: the bound `excess <= floor` of that test rejects the two mistakes an 8-channel / distinct-rows
stem launcher can make that its other assertions would not name -- a pad channel that is not zero, and output row r read from source row
r instead of r % src_rows (the full output; the distinct rows r < src_rows are the same under both) -- on every case of the test where
the mistake can be made (a pad channel exists: 5 channels at pitch 8, every case at pitch 16; src_rows > 0), for both 16-bit types.  A
16-bit result that is the correctly rounded mutant is held to the bound exactly as the kernel's output is; every mutant must be
rejected: kept fraction 100 %."""
import pytest

from tests import sample_op_refs as S
from tests.test_gpu_stem8 import CHANNELS, GEOMS, NB, reference, sources


def mutant_pad_channel(ref, c):
    out = ref.clone()
    out[:, 1:-1, 1:-1, c] = 2.0 ** -6  # one pad channel carries a small constant
    return out


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_the_bound_rejects_a_nonzero_pad_channel_and_ignored_src_rows(dtname):
    dt = S.DTYPES[dtname]
    cases = kept = 0
    for geom, (hw, uhw) in GEOMS.items():
        for ch in CHANNELS.values():
            cin = sum(ch)
            for src_rows in (0, 2):
                srcs = [s.double() for s in sources(ch, hw, src_rows if src_rows else NB)]
                rows = src_rows if src_rows else NB
                for pitch in (8, 16):
                    ref = reference(srcs, uhw, src_rows, pitch)
                    excess, floor = S.excess_floor(S.round16(ref, dt), ref, dt)  # the reference itself, rounded, meets the bound
                    assert excess <= floor
                    mutants = []
                    pad = cin if pitch == 8 else cin + 1
                    if pad < pitch:
                        mutants += [("pad channel, full", mutant_pad_channel(ref, pad), ref),
                                    ("pad channel, distinct rows", mutant_pad_channel(ref, pad)[:rows], ref[:rows])]
                    if src_rows:
                        mutants.append(("src_rows ignored", reference(srcs, uhw, src_rows, pitch, "src_rows_ignored"), ref))
                    for tag, bad, want in mutants:
                        excess, floor = S.excess_floor(S.round16(bad, dt), want, dt)
                        print(f"{dtname} pitch {pitch} {geom} {ch} src_rows {src_rows} {tag}: excess {excess:.3e} floor {floor:.3e}")
                        cases += 1
                        kept += bool(excess > floor)
    # pad-channel mutants: 2 geometries x 2 src_rows x (3 channel sets at pitch 16 + 1 at pitch 8) x 2; src_rows: 2 x 3 x 2 pitches
    assert cases == 32 + 12 and kept == cases, (kept, cases)
