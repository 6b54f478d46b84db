"""The DiT / Latte oracle (oracle/dit_oracle.py) pinned to the reference's own DiTResNet,
DiTNet and LatteNet at grids the patch does not divide (tests/golden/dit_anygrid.npz, made
by tests/golden/make_golden_dit_anygrid.py): the patch embed's zero pad at the end of each
axis and unpatchify2's centre crop.  Thresholds of tests/test_oracle_dit.py."""
import pytest

import dit_anygrid_cases as AC
from goldutil import golden_err


@pytest.fixture(scope="module")
def state():
    return {tag: (AC.build(tag).state_dict(), AC.tables(tag)) for tag in AC.NETS}


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("tag", list(AC.NETS))
def test_oracle_vs_reference(golden, state, tag, case):
    g = golden("dit_anygrid")
    sd, tabs = state[tag]
    x, t, lab, gr = AC.inputs(tag, case)
    x.requires_grad_()
    y = AC.oracle(tag, sd, x, t, lab, tabs)
    (y.real * gr.real + y.imag * gr.imag).sum().backward()
    assert golden_err(g, AC.key(tag, case) + "y", y) < 1e-5
    assert golden_err(g, AC.key(tag, case) + "dx", x.grad) < 1e-5
