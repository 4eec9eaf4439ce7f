"""The matrix-response inverse pass (csrc/fb_inv_chan_matrix.hip) streams 32 bytes of response per bin through registers that
the scalar form spends on its chirp; the four instantiations the headline geometry's shape takes -- k_inv_chan<12, 8 | 12, 2> (full
tiles) and <12, 8 | 12, -1> (tile shape from the geometry) -- must exist in the SHIPPED library, use no scratch memory and at
most 256 VGPRs.  Read from the code-object metadata as tests/test_kernel_resources.py does.  CPU only: nothing is launched."""
import pytest

from test_kernel_resources import kernels  # noqa: F401  (fixture)

HEADLINE_SHAPED = ["k_inv_chan<12, 8, 2>", "k_inv_chan<12, 12, 2>", "k_inv_chan<12, 8, -1>", "k_inv_chan<12, 12, -1>"]
# (no spill is tolerated: a tolerated one would be listed here with its byte count, the reason and the measured cost)
TOLERATED = {}


@pytest.mark.parametrize("name", HEADLINE_SHAPED)
def test_matrix_inverse_pass_uses_no_scratch(kernels, name):  # noqa: F811
    assert name in kernels, "%s is not in the library" % name
    kd = kernels[name]
    scratch = int(kd.get(".private_segment_fixed_size", 0))
    print(name, "vgprs", kd.get(".vgpr_count"), "scratch", scratch)
    assert scratch <= TOLERATED.get(name, 0), "%s uses %d bytes of scratch per lane (%d VGPRs)" % (name, scratch, kd.get(".vgpr_count", -1))
    assert int(kd.get(".vgpr_count", 0)) <= 256


def test_every_scalar_form_has_a_matrix_form(kernels):  # noqa: F811
    """k_inv_chan<I, 8, .> and <I, 12, .> for every I and tile form the plain scalar pass <I, 0, .> has"""
    scalar = [n for n in kernels if n.startswith("k_inv_chan<") and n.split(", ")[1] == "0"]
    assert len(scalar) >= 20
    for n in scalar:
        logf, _, logt = n[len("k_inv_chan<"):-1].split(", ")
        for epip in (8, 12):
            assert "k_inv_chan<%s, %d, %s>" % (logf, epip, logt) in kernels, (n, epip)
