"""CPU: the switch and the query of the background pass over the embedding table (mmda_misa_set_embed_background,
mmda_misa_embed_background_active) refuse bad arguments with MMDA_EINVAL and launch nothing; the Python wrappers exist."""
from mmda_amd import _lib, make_config, MISA

EINVAL = -1


def _model():
    return MISA(make_config(vocab_size=50))


def test_setter_refuses_null_and_bad_arguments():
    lib = _lib.load()
    assert lib.mmda_misa_set_embed_background(None, 1, 0) == EINVAL
    m = _model()
    for on, wgs in ((0, 0), (1, 0), (1, 8), (1, 4096), (0, 16)):
        assert lib.mmda_misa_set_embed_background(m._h, on, wgs) == 0
    for on, wgs in ((2, 0), (-1, 0), (1, -1), (1, 4097), (0, -5)):
        assert lib.mmda_misa_set_embed_background(m._h, on, wgs) == EINVAL


def test_query_refuses_null_and_reads_zero_before_any_step():
    lib = _lib.load()
    assert lib.mmda_misa_embed_background_active(None) == EINVAL
    m = _model()
    assert lib.mmda_misa_embed_background_active(m._h) == 0
    assert lib.mmda_misa_set_embed_background(m._h, 1, 0) == 0        # the switch alone runs nothing
    assert lib.mmda_misa_embed_background_active(m._h) == 0


def test_python_wrappers():
    m = _model()
    m.set_embed_background(True)
    m.set_embed_background(True, workgroups=16)
    m.set_embed_background(False)
    assert m.embed_background_active() is False
    for bad in (-1, 5000):
        try:
            m.set_embed_background(True, workgroups=bad)
        except _lib.MMDAError:
            continue
        raise AssertionError(f"workgroups={bad} was accepted")
