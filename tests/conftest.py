import os
import sys

# CPU runs: engines, gloo ranks and reference ops each start an OpenMP pool; with
# one pool per process sized to every core, multi-process tests oversubscribe the
# CPUs and spin-waiting pools slow them ~10x. An explicit setting (the GPU box
# exports 16) wins.
os.environ.setdefault("OMP_NUM_THREADS", "2")

import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) GPU")
    config.addinivalue_line("markers", "slow: long-running test")


def pytest_collection_modifyitems(config, items):
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:  # pragma: no cover
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU available")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture
def uds_dir():
    """A directory for Unix-socket files. sockaddr_un.sun_path holds 107 bytes, and
    pytest's tmp_path under a deep TMPDIR plus the test's name is longer than that
    (bind fails with "AF_UNIX path too long"), so sockets get a directory of their
    own, 18 characters below the first temp root that leaves room for the file's
    name, removed afterwards."""
    import pathlib
    import shutil
    import tempfile

    for base in (tempfile.gettempdir(), "/tmp", "/dev/shm"):
        if len(base) <= 60 and os.path.isdir(base) and os.access(base, os.W_OK | os.X_OK):
            d = tempfile.mkdtemp(prefix="llmd-uds-", dir=base)
            break
    else:
        pytest.fail("no short writable directory for a Unix socket")
    try:
        yield pathlib.Path(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(autouse=True)
def _seed_torch():
    """This PyTorch build seeds its default generator randomly per process, and
    many tests build random-init tiny models whose greedy outputs are compared
    across parallel layouts (TP / EP / DBO sum in other orders): a fixed seed
    keeps those models - and any near-ties in their logits - the same every run."""
    import torch

    torch.manual_seed(int(os.environ.get("LLMD_TEST_SEED", "0")))
    yield
