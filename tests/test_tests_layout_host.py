"""The suite's own layout: helpers live in plain modules (gpu_support.py, stream_compose.py, the *_ref.py restatements, ...), and no
module under tests/ imports a test module for them, which would tie the modules' import order and globals together."""
import os
import re

from conftest import REPO


def test_no_module_under_tests_imports_a_test_module():
    imports = re.compile(r"^\s*(from\s+test_\w+\s+import\b|import\s+(.*,\s*)?test_\w+)", re.M)
    tests = os.path.join(REPO, "tests")
    seen = 0
    for name in sorted(os.listdir(tests)):
        if name.endswith(".py"):
            seen += 1
            found = imports.search(open(os.path.join(tests, name)).read())
            assert found is None, (name, found.group(0))
    assert seen > 50
    for line in ("from test_gpu_dpc import H, W", "    from test_formats import write_dataset", "import test_validate as TV", "import os, test_host"):
        assert imports.search(line), line
    for line in ("from stream_compose import compose", "import stream_ref", "from gpu_support import same as test_same", "# from test_gpu_dpc import H"):
        assert not imports.search(line), line
