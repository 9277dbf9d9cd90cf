"""A short, seeded run of the randomised forward fuzz (tests/analysis/fuzz_forward.py): random ragged shapes around the
kernel-selection thresholds x arithmetic mode x tuning knobs x padding, judged against the fp64 truth with the
reference's own fp32 error as the yardstick; outputs-only and reruns bit-identical.  The long form is the script."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "analysis"))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [11, 12])
def test_seeded_forward_fuzz_has_no_violation(seed):
    import fuzz_forward
    lines = []
    bad = fuzz_forward.run(cases=10, seed=seed, max_tokens=2500, log=lines.append)
    assert bad == 0, "\n".join(line for line in lines if line.startswith("BAD"))


def test_forward_fuzz_with_mixed_tile_gemm_plans_and_tile_bit_identity():
    """the mixed-tile fp32 GEMM (the default choice of every mid-size Linear, with the FOLD / STATS epilogues) was outside
    the forward fuzz's knob and size space.  Every second case here is an 18 k .. 40 k-token alignment (whole rounds of 512 tiles plus
    a tail), gemm_tile drawn from 0..4, and on those cases uniform 128x128 tiles and mixed plans must give the same bits."""
    import fuzz_forward
    lines = []
    bad = fuzz_forward.run(cases=4, seed=61, max_tokens=2500, log=lines.append, big_every=2)
    assert bad == 0, "\n".join(line for line in lines if line.startswith("BAD"))
    assert sum(1 for line in lines if line.startswith("ok") and int(line.split("R=")[1].split()[0]) * int(line.split("C=")[1].split()[0]) >= 18000) == 2, lines


def test_tall_narrow_alignments_where_the_reference_itself_is_noisy():
    """R >> C: tied logits are sums over R x 64 products; the reference's blocked CPU sgemm is up to 7e-3 off the truth on
    the maps there, the exact path (512-term chains) stays at 1e-4 .. 3e-4."""
    import fuzz_forward
    lines = []
    bad = fuzz_forward.run(fixed=[(300, 8), (257, 16), (400, 12)], fixed_mode="f32", fixed_knobs={"ln_fold": 1}, log=lines.append)
    assert bad == 0, "\n".join(lines)


@pytest.mark.parametrize("seed", [21, 22])
def test_seeded_kernel_fuzz_has_no_violation(seed):
    """fp32 kernel entry points on strided views with ragged sizes and every epilogue combination vs fp64 torch arithmetic
    (tests/analysis/fuzz_kernels.py)."""
    import fuzz_kernels
    lines = []
    bad = fuzz_kernels.run(cases=20, seed=seed, log=lines.append)
    assert bad == 0, "\n".join(line for line in lines if line.startswith("BAD"))


@pytest.mark.parametrize("seed", [31, 32])
def test_seeded_attention16_fuzz_has_no_violation(seed):
    """16-bit attention entry points (row_logits16, softmax_rows_planes, row_apply16, col_attn16 and its prescaled entry) at
    shapes biased to the dispatch thresholds up to 1024, every mode / knob / mask / plane-output combination, on plane views
    inside NaN-filled buffers, vs fp64 (tests/analysis/fuzz_kernels.py run16)."""
    import fuzz_kernels
    lines = []
    bad = fuzz_kernels.run16(cases=15, seed=seed, log=lines.append)
    assert bad == 0, "\n".join(line for line in lines if line.startswith("BAD"))
