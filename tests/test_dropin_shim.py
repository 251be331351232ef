"""`bevrender_amd.dropin.install()` in front of the reference's imports of its own `model` and
`loss` packages must hand the reference this repo's model and retrieval losses and leave the rest of its `loss` package
alone.  Self-contained: the test lays out a stand-in checkout in a temporary directory -- a `model` package and a `loss`
package with one module per loss, each defining a placeholder class under the reference's name -- and runs the imports
the contract names from there, so that without the shim every name would resolve to the stand-in.  CPU only, in a
child process (the aliases must not leak into the test session).  Third-party packages the image lacks (wandb,
torchvision, timm, pytorch_metric_learning, yourdfpy) are stubbed as empty modules."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the names INTEGRATION.md section 1 routes: module -> class.  MINE come from this package after install(), THEIRS stay
# the checkout's own
MINE = {"loss.contrastive_loss": "ContrastiveLoss", "loss.lift_loss": "LiftedStructureLoss",
        "loss.triplet_loss_metric": "TripletLossMetricLearning", "model.bevrender": "BEVRender"}
THEIRS = {"loss.mse_loss": "MSELoss", "loss.l1_loss": "L1Loss", "loss.cross_entropy_loss": "CrossEntropyLoss"}


def _stand_in_checkout(root):
    """model/ and loss/ packages whose modules each define a placeholder class of the reference's name."""
    for pkg in ("model", "loss"):
        os.makedirs(os.path.join(root, pkg))
        open(os.path.join(root, pkg, "__init__.py"), "w").close()
    for mod, cls in {**MINE, **THEIRS, "model.SCA_deform_attn": "SCADeformableAttention"}.items():
        with open(os.path.join(root, *mod.split(".")) + ".py", "w") as fh:
            fh.write(f"class {cls}:\n    pass\n")


def test_reference_import_block_resolves_to_this_package(tmp_path):
    ref = str(tmp_path / "checkout")
    _stand_in_checkout(ref)
    block = "\n".join(f"from {m} import {c}" for m, c in {**THEIRS, **MINE}.items())
    code = textwrap.dedent(f"""
        import importlib.abc, importlib.machinery, os, sys, types
        sys.path.insert(0, {ROOT!r})

        ABSENT = ("wandb", "torchvision", "timm", "pytorch_metric_learning", "yourdfpy")

        class Stub(types.ModuleType):
            __path__ = []
            def __getattr__(self, name):
                if name.startswith("__"):
                    raise AttributeError(name)
                return type(name, (), {{}})

        class Finder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
            def find_spec(self, fullname, path, target=None):
                if fullname.split(".")[0] in ABSENT:
                    return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
            def create_module(self, spec):
                return Stub(spec.name)
            def exec_module(self, module):
                pass

        sys.meta_path.insert(0, Finder())
        import bevrender_amd.dropin
        bevrender_amd.dropin.install()

        os.chdir({ref!r})
        sys.path.insert(0, {ref!r})
        ns = {{}}
        exec(compile({block!r}, "import block", "exec"), ns)
        mine = lambda o: o.__module__.startswith("bevrender_amd.")
        assert mine(ns["BEVRender"]), ns["BEVRender"].__module__
        for n in ("ContrastiveLoss", "LiftedStructureLoss", "TripletLossMetricLearning"):
            assert mine(ns[n]), (n, ns[n].__module__)
        for n in ("MSELoss", "L1Loss", "CrossEntropyLoss"):
            f = sys.modules[ns[n].__module__].__file__
            assert ns[n].__module__.startswith("loss.") and f.startswith({ref!r}), (n, f)
        import model.SCA_deform_attn as m
        assert m.__name__ == "bevrender_amd.model.SCA_deform_attn"
        print("SHIM-OK")
    """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SHIM-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
