"""tests/golden/node_surface_adv.json: the contracts of the reference's advanced (Ad) node classes, captured from the classes
themselves, and the node types its float_adv*.json example graphs use.

BUILD-CONTAINER ONLY (tools/ref_import.py: the reference tree is imported with stand-ins for the packages it needs).  The
fixture holds names, types, defaults, ranges and return tuples only - tooltips are prose, not contract, and are dropped.

    python tools/make_adv_surface_golden.py
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def strip(o):
    if isinstance(o, dict):
        return {k: strip(v) for k, v in o.items() if k != "tooltip"}
    if isinstance(o, (list, tuple)):
        return [strip(v) for v in o]
    return o


def node_classes(mod):
    return {name: c for name, c in vars(mod).items() if isinstance(c, type) and hasattr(c, "UNIQUE_NAME") and c.__module__ == mod.__name__}


def main():
    adv = ref_import.import_ref("src.nodes.nodes_adv")
    classes = {}
    for name, c in node_classes(adv).items():
        classes[name] = dict(INPUT_TYPES=strip(c.INPUT_TYPES()), RETURN_TYPES=list(c.RETURN_TYPES), RETURN_NAMES=list(c.RETURN_NAMES),
                             FUNCTION=c.FUNCTION, CATEGORY=c.CATEGORY, UNIQUE_NAME=c.UNIQUE_NAME, DISPLAY_NAME=c.DISPLAY_NAME,
                             SUFFIX=adv.SUFFIX)
    # every node type the reference registers (the four modules its __init__.py hands to register_nodes) ...
    registered = set()
    for m in ("nodes", "nodes_adv", "nodes_vadv", "nodes_vadv_loader"):
        registered |= {c.UNIQUE_NAME for c in node_classes(ref_import.import_ref("src.nodes." + m)).values()}
    # ... that occurs in an advanced example graph (the other types there are ComfyUI's own and other packs')
    used = set()
    for path in sorted(glob.glob(os.path.join(ref_import.REF_ROOT, "example_workflows", "float_adv*.json"))):
        with open(path) as f:
            graph = json.load(f)
        stack = [graph]
        while stack:  # nodes of the graph and of its subgraph definitions
            o = stack.pop()
            if isinstance(o, dict):
                if isinstance(o.get("type"), str) and "id" in o:
                    used.add(o["type"])
                stack.extend(o.values())
            elif isinstance(o, list):
                stack.extend(o)
    out = dict(classes=classes, workflow_node_types=sorted(used & registered))
    with open(os.path.join(GOLD, "node_surface_adv.json"), "w") as f:
        json.dump(out, f, indent=1, default=str)
    print("wrote node_surface_adv.json: %d classes, workflow node types %s" % (len(classes), out["workflow_node_types"]))


if __name__ == "__main__":
    main()
