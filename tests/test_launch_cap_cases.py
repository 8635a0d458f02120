"""Host checks of the launch-cap case table (tests/launch_cap_cases.py): at every CU count the device tests may meet,
every case takes the path it names and holds at most 1 GiB of device buffers.  No device."""
import pytest

from tests import launch_cap_cases as LC

CASES = LC.cases()


@pytest.fixture(scope="module")
def k():
    return LC.constants()


def test_the_table_names_every_case_once():
    names = [c.name for c in CASES]
    assert len(names) == len(set(names)) and all(c.where.endswith(".hip") and c.cap for c in CASES)


@pytest.mark.parametrize("cu", LC.CU_COUNTS)
@pytest.mark.parametrize("case", CASES, ids=LC.case_id)
def test_case_crosses_its_cap_under_one_gib(case, cu, k):
    shape = case.shape(cu, k)
    assert case.crosses(cu, k), f"{case.name} at {cu} CUs ({shape}) does not take: {case.cap}"
    n = case.bytes(cu, k)
    assert 0 < n <= LC.GIB, f"{case.name} at {cu} CUs ({shape}): {n} bytes of device buffers"


def test_colored_noise_itself_never_fills_a_grid(k):
    """ops.colored_noise cuts a batch into pieces of MAX_ROWS div 2 pairs: no piece holds more rows than the grid's y
    dimension, so the row loops of the pair kernels are reached through the library's entries alone."""
    for L in (2, LC.COLORED_L, 1000, 1 << 20):
        assert LC.colored_piece_rows(L, k) <= LC.RNG_MAX_ROWS_Y
    first, P = LC.colored_pairs(LC.COLORED_FIRST_ROW, LC.COLORED_B)
    assert first == LC.COLORED_FIRST_ROW // 2 and 2 * (first + P) >= LC.COLORED_FIRST_ROW + LC.COLORED_B


def test_the_slice_plan_is_the_library_s():
    """noise_gen_slices against syg_fx_add_noise_gen_work_bytes, which sizes (B S + B) double2."""
    from sygnals_amd import ops
    for B, L in [(1, 16385), (3, 65537), (31, 64 * 4096 + 1), (32, 64 * 4096 + 1), (2048, 16385), (5, 1 << 20)] + \
            [(B, L) for B, L, _ in LC.GEN_SLICE_CASES]:
        S = LC.noise_gen_slices(B, L)[0]
        assert ops._work_bytes("syg_fx_add_noise_gen_work_bytes", B, L) == (B * S + B) * 16, (B, L, S)
