#!/usr/bin/env python3
"""Records what PIL itself gives on every case of tests/preprocess_ref.py into tests/golden/preprocess_pil.safetensors: Image.resize
with BOX / BILINEAR / BICUBIC, center_crop_arr, Resize + CenterCrop, Resize((S, S)) and crop + resize (+ flip), uint8 [h, w, 3]
per image under the key "<case>.<image index>".  Only outputs are stored: the inputs are regenerated from their seeds.  Run it
where Pillow is installed (the version goes into the file's metadata); the tests then pin the numpy restatement, and through it
the kernels, on machines without PIL.

    python tools/record_preprocess_golden.py [--out tests/golden/preprocess_pil.safetensors]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "preprocess_pil.safetensors"))
    a = ap.parse_args()
    import PIL
    from safetensors.numpy import save_file

    import preprocess_ref as R
    tensors = {}
    for name, case in R.cases().items():
        for i, out in enumerate(R.pil_expected(case)):
            tensors[f"{name}.{i}"] = np.ascontiguousarray(out, dtype=np.uint8)
    save_file(tensors, a.out, metadata={"pillow": PIL.__version__, "cases": str(len(R.cases()))})
    print(f"{len(tensors)} outputs of {len(R.cases())} cases, Pillow {PIL.__version__} -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
