import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "metaquest-3d-reconstruction_amd"), os.path.join(ROOT, "oracle"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through libmqr_hip.so)")


@pytest.fixture(scope="session")
def golden_dir():
    return os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="session")
def confidence_golden(golden_dir):
    """The confidence golden vectors as one read-only mapping (<seq>_<field> -> array).  They are
    stored one file per sequence, confidence_golden_<seq>.npz, so that each stays under 1 MiB."""
    import numpy as np
    out = {}
    for seq in ("sphere", "room"):
        with np.load(os.path.join(golden_dir, f"confidence_golden_{seq}.npz")) as z:
            for k in z.files:
                out[k] = z[k]
                out[k].setflags(write=False)
    return out
