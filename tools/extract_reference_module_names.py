#!/usr/bin/env python3
"""Extract, per reference module, the public top-level function / class names into a JSON fixture (parsed with
``ast``, never imported).

``tests/test_module_paths.py`` imports ``torchmetrics_amd.<module>`` for every recorded module and checks that each
recorded name resolves there, so the test needs no reference tree at run time.

Usage: ``python tools/extract_reference_module_names.py --ref <reference checkout>`` ->
``tests/golden/reference_module_names.json``.
"""
import argparse
import ast
import json
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def extract(ref: Path) -> dict:
    out = {}
    src = ref / "src" / "torchmetrics"
    for path in sorted(src.rglob("*.py")):
        rel = str(path.relative_to(src))[:-3].replace("/", ".")
        if rel.endswith("__init__"):
            rel = rel[: -len(".__init__")] if rel != "__init__" else ""
        names = [n.name for n in ast.parse(path.read_text()).body
                 if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and not n.name.startswith("_")]
        out[rel] = names
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "reference_module_names.json"))
    args = ap.parse_args()
    data = extract(Path(args.ref))
    Path(args.out).write_text(json.dumps(data, indent=0, sort_keys=True))
    print(f"{len(data)} modules -> {args.out}")


if __name__ == "__main__":
    main()
