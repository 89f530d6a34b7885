"""bench.py --dump-outputs on the CPU: the writer's files, dtypes and shapes (the GPU run is in
tests/test_gpu_bench_contract.py), and the arguments it refuses."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("_bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _Result:
    def __init__(self, success, score, bbox):
        self.success, self.score, self.bbox = success, score, bbox


def test_dump_outputs_writes_float_arrays_in_stream_order(tmp_path):
    bench = _bench()
    res = [_Result(True, 0.6789, [294, 256, 64, 64]), _Result(False, 0.125, [1, 2, 3, 4])]
    bench.dump_outputs(str(tmp_path / "out"), res)
    bbox, score, success = (np.load(tmp_path / "out" / f"{n}.npy") for n in ("bbox", "score", "success"))
    assert bbox.dtype == np.float64 and bbox.tolist() == [[294, 256, 64, 64], [1, 2, 3, 4]]
    assert score.dtype == np.float32 and score.tolist() == [np.float32(0.6789), 0.125]
    assert success.dtype == np.float32 and success.tolist() == [1.0, 0.0]


def test_plain_is_the_default_and_steps_must_be_positive():
    bench = _bench()
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "0"])
    assert a.full is False and a.dump_outputs == "" and a.steps == 5
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full is True
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
