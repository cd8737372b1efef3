"""Every compiled (KC, R) body of gf_mac_ragged_rows_kernel on the MI355X,
against the CPU oracle.

One test id per KC of mac_bodies.COMPILED; it loops over
test_gpu_mac_bodies.rebuild_codes(KC) and sends each code through
Codec.rebuild_ragged with per-block patterns on list C (straddles, a
three-tile block, zero sizes) and on the code's own H(cap): cap blocks of 64
bytes and one of two tiles, so that the first tile builds as many table sets
as the plan allows and the tile behind it straddles.  Every failing code is
reported, not the first."""
import pytest

import mac_bodies as B
import test_gpu_ragged_rebuild as RR
from test_gpu_bounds import Cases
from test_gpu_mac_bodies import KCS, KC_IDS, attempt, rebuild_codes

pytestmark = pytest.mark.gpu


def test_the_sweep_reaches_every_compiled_body():
    reached = {B.body(k, e) for KC in KCS for (k, m, e) in rebuild_codes(KC)}
    assert reached == set(B.COMPILED)


@pytest.mark.parametrize("KC", KCS, ids=KC_IDS)
def test_ragged_rebuild(codec, O, KC):
    cases = Cases()
    for k, m, e in rebuild_codes(KC):
        for name in ("C", "H0"):
            attempt(cases, "rs%d_%d e=%d %s" % (k, m, e, name), RR.checked, codec, O, name, k, m, e)
    cases.done()
