"""GPU: tools/pipeline_y4m.py with its ME stages taken by svt_hip_motion_estimate_frame (Pipeline(me_frame=True)) against the same
pipeline on the stage calls, picture by picture: equal search-area origins, SADs and vectors for every SB and PU, and equal digests
of everything both passes produce - issued from Python and as a captured graph that reuses the call's output buffers."""
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = 5                  # the graph is captured on the third picture and replayed for the fourth and fifth


def load_tool():
    spec = importlib.util.spec_from_file_location("pipeline_y4m", os.path.join(ROOT, "tools", "pipeline_y4m.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def run(tool, dsp, path, **kw):
    """-> per picture after the first: (area origin, SADs, vectors) as host tensors, and the digest"""
    p = tool.Pipeline(dsp, path, **kw)
    rows = []
    while True:
        o = p.step()
        if o is None:
            break
        torch.cuda.synchronize()
        if "me_sad" not in o:
            continue
        origin = o["me_area_origin"] if "me_area_origin" in o else o["me_area"][:, :2]
        rows.append((origin.cpu().clone(), o["me_sad"].cpu().clone(), o["me_mv"].cpu().clone(), tool.digest_of(o)))
    assert kw.get("use_graph", False) == (p.graph is not None)
    p.pi.close()
    return rows


def test_the_pipeline_on_the_frame_call_equals_the_pipeline_on_the_stage_calls(dsp, tmp_path):
    tool = load_tool()
    path = str(tmp_path / "pan.y4m")
    tool.synthetic_clip(path, 320, 192, NF, pan=(4, 4))
    want = run(tool, dsp, path)
    assert len(want) == NF - 1 and (want[0][2] != 0).any()
    for use_graph in (False, True):
        got = run(tool, dsp, path, me_frame=True, use_graph=use_graph)
        assert len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            for k, name in enumerate(("area origin", "me_sad", "me_mv")):
                assert torch.equal(g[k], w[k]), (use_graph, i, name)
            shared = set(g[3]) & set(w[3])
            assert {"me_sad_sum", "me_mv_sum", "ois_best_sum", "enc_digest"} <= shared
            assert all(g[3][k] == w[3][k] for k in shared), (use_graph, i)
