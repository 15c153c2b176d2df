"""The staged host path (DHQR_HOSTIO=1, csrc/dhqr_hostio.h) on the EMULATED library, against the plain form, bit for bit.

dhqr_qr_f64 reads DHQR_HOSTIO once per process, so each setting runs in a child process (tests/helpers/schedule_child.py,
the case list "emu") that prints a SHA-256 of every output.  The staged form uploads through four rotating pinned buffers,
factors the same device copy with the same dhqr_factor_f64 and downloads every column block behind its panel's commit, so
hA, halpha and hx must equal the plain form's exactly.  Streams, events and host functions are synchronous on the emulator:
this cannot see a race (test_gpu_schedule.py makes the same comparison on the GPU); it sees the bookkeeping -- buffer
rotation, the partial last block, `done`, the resume rule after a rejected panel, a capacity kept between calls."""
import pytest

from schedule_helpers import compare_hostio, hostio_case_names, run_hostio_children


@pytest.fixture(scope="module")
def children(emulated_so):
    return run_hostio_children(emulated_so, "emu", timeout=900)


@pytest.mark.parametrize("case", hostio_case_names("emu"))
def test_staged_host_io_equals_plain_emulated(children, case):
    # 1e-9 relative: the bound on x of test_host_entry_points_on_guarded_layouts (test_gpu_layouts.py)
    compare_hostio(*children, x_tol=1e-9, only=case)
