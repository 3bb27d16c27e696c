"""Every reference module path resolves, and carries the public names the reference defines there.

The (module, names) pairs are the fixture ``tests/golden/reference_module_names.json``
(``tools/extract_reference_module_names.py``: parsed with ``ast`` from the reference's sources).
"""
import importlib
import json
import os

import pytest

from torchmetrics_amd import _module_aliases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_module_names.json")


def _reference_modules():
    with open(GOLDEN) as f:
        data = json.load(f)
    return [("torchmetrics_amd" + ("." + rel if rel else ""), names) for rel, names in sorted(data.items())]


@pytest.mark.parametrize("alias", sorted(_module_aliases.aliases()))
def test_alias_imports(alias):
    mod = importlib.import_module(alias)
    assert mod.__name__ == alias


def test_reference_public_names_resolve():
    modules = _reference_modules()
    assert len(modules) > 100, len(modules)
    missing = []
    for mod_name, names in modules:
        mod = importlib.import_module(mod_name)
        missing += [f"{mod_name}.{n}" for n in names if not hasattr(mod, n)]
    assert not missing, missing
