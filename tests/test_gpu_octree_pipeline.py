"""GPU: the whole extractor on frames whose candidate lists the octree's count tables give up on, so that k_octree_redo runs inside the pipeline
on known levels (tests/octree_device_cases.py; the levels are re-established on the CPU by tests/test_octree_table_model.py): every stage against
the oracle, graph replay, the iterative form alone (ORBHIP_OCTREE=iterative), and an image whose levels differ in nIni."""
import numpy as np
import pytest

import octree_device_cases as D
from test_gpu_orb import _compare_frame

pytestmark = pytest.mark.gpu


def _same(a, b, frames):
    for f in frames:
        assert a[f][2] == b[f][2] and a[f][0].tobytes() == b[f][0].tobytes() and a[f][1].tobytes() == b[f][1].tobytes(), f


@pytest.fixture(scope="module")
def pipe(gpu_ctx):
    """24 VGA frames (the spatial permutation is on; 8 x 24 lists are three workgroups of k_octree_redo), the constructed images at frames 0, 7, 8
    and 23, extracted once in the form the environment selects."""
    import orbhip
    import oracle_bind as ob
    imgs = D.pipeline_images(orbhip.synth_frames)
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    got = ext.extract_host(imgs)
    yield imgs, ext, ob.OracleExtractor(1000, 1.2, 8, 20, 7), got
    ext.close()


def test_flagged_levels_inside_the_pipeline(pipe):
    imgs, ext, ora, got = pipe
    assert len(imgs) == D.PIPE_FRAMES
    for f in sorted(D.PIPE_CONSTRUCTED) + list(D.PIPE_ORDINARY):
        assert _compare_frame(ext, ora, imgs, f, (0, 1000), got) > 0


def test_flagged_levels_under_graph_replay(gpu_ctx, pipe):
    import orbhip
    imgs, _, _, got = pipe
    graph = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    graph.set_graph_mode(True)
    for _ in range(2):                                       # capture, then replay
        _same(graph.extract_host(imgs), got, range(D.PIPE_FRAMES))
    graph.close()


def test_iterative_form_alone_gives_the_same_bytes(gpu_ctx, pipe, monkeypatch):
    import orbhip
    imgs, _, _, got = pipe
    monkeypatch.setenv("ORBHIP_OCTREE", "iterative")         # read when the extractor reserves
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    _same(ext.extract_host(imgs), got, range(D.PIPE_FRAMES))
    ext.close()


def test_levels_of_different_n_ini(gpu_ctx):
    """700 x 480: one root on the large levels, two on the small ones; the tables are sized for two and indexed with the level's own."""
    import orbhip
    import oracle_bind as ob
    imgs = D.wide_pair(orbhip.synth_frames)
    ext = orbhip.Extractor(gpu_ctx, 1000, 1.2, 8, 20, 7)
    ora = ob.OracleExtractor(1000, 1.2, 8, 20, 7)
    got = ext.extract_host(imgs)
    n_ini = [D.n_ini_of(w - 32, h - 32) for w, h in (ext.level_dims(l) for l in range(8))]
    assert ext.level_dims(0) == (700, 480) and ext.level_dims(3) == (405, 278)
    assert n_ini[0] == 1 and n_ini[3:] == [2] * 5
    for f in range(2):
        assert _compare_frame(ext, ora, imgs, f, (0, 1000), got) > 0
    ext.close()
