"""``ecb_downsample.downsample`` on tensors still in flight (``tests/inflight.py``): the counts a kernel queued on torch's current stream --
the default one or a side stream -- has not written yet when the wrapper is called, through every conversion the wrapper can be made to
queue, and the inputs reused the moment it returns.  The case runs through ``test_gpu_inflight_tensors.run_case`` as every other wrapper's
does: the result is the checker's, it is that of the same call on finished tensors, and it is not the decoy's."""
import numpy as np
import pytest

from alntools_amd import ecb_downsample as ed

import downsample_checker as dc
import inflight as fl
import test_gpu_inflight_tensors as ti
from inflight import Input

pytestmark = pytest.mark.gpu
SEED = 9


def entry_downsample():
    """The matrices of the other cases: the counts have a decoy (other valid counts), the arrays that index and the targets keep their
    content; half of every sample's real reads are asked for, one column is copied and one emptied."""
    m, T, H, S = ti._matrix(1)
    _, dn = ti._decoys(m, H, 31, 1)
    E = m.num_reads
    target = dc.totals(m) // 2
    target[2], target[5] = -1, 0
    ins = ti._six(m, None, dn)[3:] + [Input("tg", target.astype(np.int64))]
    return ti.Entry(ins, lambda v, _: ed.downsample(v["pn"], v["xn"], v["dn"], E, v["tg"], seed=SEED),
                    lambda a: list(dc.downsample(a["pn"], a["xn"], a["dn"], E, a["tg"], SEED)))


MODES = [mode for mode in fl.MODES]


@pytest.mark.parametrize("mode", MODES)
def test_downsample_on_tensors_in_flight_on_the_current_stream(mode, monkeypatch):
    monkeypatch.setitem(ti.WRAPPERS, "downsample", (entry_downsample, ti.ALL3))
    ti.run_case("downsample", mode, monkeypatch)
