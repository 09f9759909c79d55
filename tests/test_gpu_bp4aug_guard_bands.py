"""fgnn_bp4aug_decode between guard bands (tests/guarded.py), in the frame of tests/test_gpu_guard_bands.py: at both bp4aug_kernel
instantiations (ibm72: the (3,3,6) rows; the others and force_generic: the loop), codes with n mod 4 = 0 .. 3, batches 0, 1, 3 and one
more than a workgroup holds, the default launch and set_launch.  Guards intact, no poison left in x_hat / z_hat / stats, outputs equal to
the restatement, inputs unchanged."""
import pytest

import bp4aug_reference as AU
from helpers import code, llr_const
from test_gpu_guard_bands import N_MOD_4, P_OF, QUATERNARY, SEED, _bp4_family_case

pytestmark = pytest.mark.gpu


def test_the_cases_cover_every_tail():
    assert {N_MOD_4[name] for name, _ in QUATERNARY} == {0, 1, 2, 3}


@pytest.mark.parametrize("restart,density", [(True, 0.3), (False, 1.0)])
@pytest.mark.parametrize("name,variant", QUATERNARY)
def test_bp4aug_decode(name, variant, restart, density):
    L = llr_const(P_OF[name])
    _bp4_family_case(name, variant,
                     lambda g, sx, sz, _: g.bp4aug_decode(sx, sz, 3, 2, 3, density, "minsum", 0.8, restart=restart, seed=SEED,
                                                          first_sample=0, llr_const=L),
                     lambda sx, sz: AU.bp4aug_decode(code(name), sx, sz, 3, 2, 3, density, "minsum", 0.8, restart=restart, seed=SEED,
                                                     first_sample=0, llr_const=L))
