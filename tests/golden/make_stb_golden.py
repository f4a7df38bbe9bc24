"""Regenerates stb_decodes.json and stb_pillow_inputs.npz of this directory: stb_image's decode of every case of
tests/test_decoders_vs_stb.py, taken from the live reference decoder (oracle/_ref/libstb_ref.so, built by `make -C oracle` where the
reference tree is present), and the Pillow-written input files of that test.

The script runs the test's own case loops with a recording stand-in for its `stb` fixture, so the labels and inputs are the test's.
The decode records are shape + SHA-256 of the RGBA bytes (null where stb_image refuses the file); the product's decoder is compared
with the live decoder on the way, so a run that finishes also means the product agrees with stb_image on every case.

    python tests/golden/make_stb_golden.py
"""
import json
import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_decoders_vs_stb as t  # noqa: E402


class _Recorder:
    def __init__(self, live):
        self.live, self.decodes = live, {}

    def __call__(self, data, what):
        assert what not in self.decodes, f"case label {what!r} is not unique"
        want = self.live(data)
        self.decodes[what] = t._record(want)
        return want


def main():
    if not os.path.exists(t._LIB):
        raise SystemExit(f"{t._LIB} is not built: make -C oracle (needs the reference tree)")
    from PIL import Image
    files = list(t.pillow_jpeg_files(Image)) + list(t.pillow_png_files(Image))
    np.savez_compressed(t.PILLOW_INPUTS, order=np.array([k for k, _ in files]), **{k: np.frombuffer(v, np.uint8) for k, v in files})
    rec = _Recorder(t._live_loader())
    with tempfile.TemporaryDirectory() as d:
        tmp = pathlib.Path(d)
        t.test_png_matrix_equals_stb_image(tmp, rec)
        t.test_png_single_filter_files_equal_stb_image(tmp, rec)
        t.test_baseline_jpeg_equals_stb_image(tmp, rec)
        t.test_pillow_written_jpeg_equals_stb_image(rec)
        t.test_pillow_written_png_equals_stb_image(rec)
        t.test_both_refuse_the_same_broken_files(tmp, rec)
    with open(t.GOLDEN, "w") as f:
        json.dump({"source": "stb_image (the reference's external/stb_image.h) through stbi_load_from_memory(..., 4); tests/golden/make_stb_golden.py",
                   "decodes": rec.decodes}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec.decodes)} decodes, {len(files)} Pillow-written inputs")


if __name__ == "__main__":
    main()
