"""TTS conditioners without a GPU: the toml front end (config_toml.load_tts_conditioners), the synthetic checkpoint's conditioner
tensors and the numpy reference of the row (tests/tts_cond_ref.py) against a float64 evaluation."""
import os

import numpy as np
import pytest

import tts_cond_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "configs", "tts-realtime.toml")
WDIR = os.environ.get("DSM_WEIGHTS_DIR", "/tmp/dsm_weights")

HEAD = """
[modules.tts]
type = "Tts"
[modules.tts.model]
text_in_vocab_size = 8001
"""


def _toml(tmp_path, body):
    p = tmp_path / "c.toml"
    p.write_text(HEAD + body)
    return str(p)


def test_the_shipped_realtime_config_declares_one_lut(dsm):
    from dsm_amd import config_toml
    descs = config_toml.load_tts_conditioners(GOLDEN)
    assert descs == [dict(name="description", type="Lut", dim=16, n_bins=31,
                          possible_values=["very_bad", "bad", "neutral", "good", "very_good"])]
    assert config_toml.load_tts_conditioners(GOLDEN, module="tts") == descs
    with pytest.raises(config_toml.ConfigError, match="Tts module"):
        config_toml.load_tts_conditioners(GOLDEN, module="asr")


def test_a_continuous_attribute_table_parses_and_file_order_is_kept(dsm, tmp_path):
    from dsm_amd import config_toml
    path = _toml(tmp_path, """
[modules.tts.model.conditioners.speed]
type = "ContinuousAttribute"
dim = 8
scale_factor = 10.0
max_period = 100
[modules.tts.model.conditioners.description]
type = "Lut"
n_bins = 4
dim = 5
possible_values = ["a", "b"]
""")
    descs = config_toml.load_tts_conditioners(path)
    assert descs == [dict(name="speed", type="ContinuousAttribute", dim=8, scale_factor=10.0, max_period=100.0),
                     dict(name="description", type="Lut", dim=5, n_bins=4, possible_values=["a", "b"])]
    assert config_toml.load_tts_conditioners(_toml(tmp_path, "")) == []


@pytest.mark.parametrize("body", [
    '[modules.tts.model.conditioners.x]\ntype = "Tensor"\ndim = 4\n',                                       # unknown type
    '[modules.tts.model.conditioners.x]\ntype = "Lut"\ndim = 4\nn_bins = 3\n',                             # no possible_values
    '[modules.tts.model.conditioners.x]\ntype = "Lut"\ndim = 4\nn_bins = 1\npossible_values = ["a", "b", "c"]\n',  # more values than rows
    '[modules.tts.model.conditioners.x]\ntype = "Lut"\ndim = 0\nn_bins = 3\npossible_values = ["a"]\n',    # dim
    '[modules.tts.model.conditioners.x]\ntype = "Lut"\ndim = 4\nn_bins = 3\npossible_values = ["a", 2]\n', # a value that is no string
    '[modules.tts.model.conditioners.x]\ntype = "ContinuousAttribute"\ndim = 8\nscale_factor = 1.0\n',     # no max_period
    '[modules.tts.model.conditioners.x]\ntype = "ContinuousAttribute"\ndim = 2\nscale_factor = 1.0\nmax_period = 10.0\n',  # half_dim - 1 = 0
    'conditioners = 3\n',                                                                                  # not a table
    '[modules.tts.model.conditioners]\nx = 3\n',                                                           # an entry that is no table
])
def test_a_malformed_table_raises(dsm, tmp_path, body):
    from dsm_amd import config_toml
    with pytest.raises(config_toml.ConfigError):
        config_toml.load_tts_conditioners(_toml(tmp_path, body))


def test_batched_asr_still_refuses_conditioners(dsm, tmp_path):
    from dsm_amd import config_toml
    src = open(os.path.join(ROOT, "tests", "golden", "configs", "stt-en_fr.toml")).read()
    name = [l for l in src.splitlines() if l.startswith("[modules.") and l.count(".") == 1][0][len("[modules."):-1]
    p = tmp_path / "stt.toml"
    p.write_text(src + f'\n[modules.{name}.model.conditioners.description]\ntype = "Lut"\nn_bins = 31\ndim = 16\npossible_values = ["a"]\n')
    with pytest.raises(config_toml.ConfigError, match="conditioners"):
        config_toml.load_batched_asr(str(p))


@pytest.fixture(scope="module")
def tensors(dsm):
    from dsm_amd import synth
    cfg = dsm.config_tts_tiny()
    path = synth.make_synth_tts_weights(cfg, WDIR, tag="tts_tiny", conditioners=CR.CONDS)
    return cfg, path, CR.cond_tensors(path)


def test_synthetic_conditioner_tensors_leave_the_other_tensors_alone(dsm, tensors):
    from dsm_amd import synth
    cfg, path, t = tensors
    d = cfg.lm.d_model
    assert os.path.basename(path) == "tts_tiny_cond-description.16.31-tail.5.4-speed.8.lm.safetensors"
    assert t["condition_provider.conditioners.description.embed.weight"].shape == (32, 16)
    assert t["condition_provider.conditioners.tail.output_proj.weight"].shape == (d, 5)
    assert t["condition_provider.conditioners.speed.learnt_padding"].shape == (1, 1, d)
    assert "condition_provider.conditioners.speed.embed.weight" not in t
    plain = synth.read_safetensors(synth.make_synth_tts_weights(cfg, WDIR, tag="tts_tiny"))
    both = synth.read_safetensors(path)
    assert set(both) - set(plain) == set(t)
    assert all(np.array_equal(both[k].view(np.uint32), v.view(np.uint32)) for k, v in plain.items())


def test_the_f32_chain_against_float64(dsm, tensors):
    """LUT rows: the chain differs from the float64 dot product by at most dim 2^-24 sum |x w|; the continuous recipe (bf16-rounded
    embedding, f32 chain) stays within the bound the GPU test uses; cosines come first and value 0 gives [1.., 0..]."""
    _, _, t = tensors
    for c in CR.CONDS[:2]:
        W = t[f"condition_provider.conditioners.{c['name']}.output_proj.weight"].astype(np.float64)
        for value in (c["possible_values"][0], c["possible_values"][-1]):
            x = t[f"condition_provider.conditioners.{c['name']}.embed.weight"][c["possible_values"].index(value)].astype(np.float64)
            got = CR.lut_row(t, c, value)
            assert got.dtype == np.float32 and got.shape == (W.shape[0],)
            assert np.all(np.abs(got - W @ x) <= c["dim"] * 2.0 ** -24 * (np.abs(W) * np.abs(x)).sum(axis=1))
            assert np.any(got != 0)
    c = CR.CONDS[2]
    e0 = CR.sin_embedding(c, 0.0)
    assert np.array_equal(e0, [1.0] * 4 + [0.0] * 4)
    e = CR.sin_embedding(c, 0.25)  # v = 2.5, a = 100^(-i/3)
    assert np.allclose(e[:4], np.cos(2.5 * 100.0 ** (-np.arange(4) / 3.0)), rtol=0, atol=1e-15)
    assert np.allclose(e[4:], np.sin(2.5 * 100.0 ** (-np.arange(4) / 3.0)), rtol=0, atol=1e-15)
    for value in (0.0, 0.25, -1.5, 3.0):
        want, bound = CR.cont_row_f64(t, c, value)
        assert np.all(np.abs(CR.cont_row_chain(t, c, value) - want) <= bound), value


def test_chain_is_a_sequential_f32_sum():
    """A case where the order of the additions is visible: 2^24 + 1 + 1 in f32 is 2^24 left to right."""
    W = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0]], dtype=np.float32)
    assert CR.chain(np.array([2.0 ** 24, 1.0, 1.0], dtype=np.float32), W).tolist() == [2.0 ** 24] * 2
    assert CR.chain(np.array([1.0, 1.0, 2.0 ** 24], dtype=np.float32), W).tolist() == [2.0 ** 24 + 2] * 2
    assert CR.bf16_round(np.float32(1.0 + 2.0 ** -8)) == np.float32(1.0)            # a tie goes to the even mantissa
    assert CR.bf16_round(np.float32(1.0 + 3 * 2.0 ** -8)) == np.float32(1.0 + 2.0 ** -6)
