"""What the case modules of the pattern ops (spmm, edge_softmax, edge_dot and the attention ops on K19, K20 and K21) share: the report
of a pricing, the build-once registry of a module's seeded cases, and the pricing, stand-in and rehearsal of a case whose ground
truth runs through torch autograd.  A case module keeps what is its own: the ground truth, the inputs and seeds of its cases
(`_build_cases`), and every assertion about them."""
import torch

import parity


def _report(what, rep):
    print(what, {k: f"{e:.2e}" for k, e in rep.items()})
    return rep


def seeded(build):
    """-> (cases, case_names) of a case module whose `build()` lists its seeded cases: built on first use, once, and shared."""
    built = []

    def cases():
        """{name: case}, built once and shared (inputs are never written to)."""
        if not built:
            built.append({c.name: c for c in build()})
        return built[0]

    def case_names(prefix=""):
        return [n for n in cases() if n.startswith(prefix)]
    return cases, case_names


class OpCase:
    """One seeded case of an op: `leaves` (the fp32-rounded float64 inputs that carry a gradient), `names` (of their gradients),
    `ref(*leaves)` (the ground truth, flattened, in the leaves' dtype) and G (the gradient of the loss <out, G>, shaped like out)."""

    def price_y64(self, out, *grads, what=None, ref=None):
        """out and the gradient of every leaf of one run against the ground truth (`ref`: another ground truth of the same leaves)
        -> (the report, the ground truth's out in fp64 shaped like out)."""
        leaves = self.leaves
        assert out.shape == self.G.shape and len(grads) == len(leaves), (self.name, out.shape, len(grads))
        for g, t in zip(grads, leaves):
            assert g.shape == t.shape, (self.name, g.shape, t.shape)
        rep, (y64, _) = parity.check_autograd(out.reshape(-1), list(grads), ref or self.ref, leaves, self.G.reshape(-1), self.names,
                                              what or self.name)
        return _report(what or self.name, rep), y64.reshape(self.G.shape)

    def price(self, out, *grads, **kw):
        """... -> the report."""
        return self.price_y64(out, *grads, **kw)[0]

    def stand_in(self, fn=None):
        """The fp32 ground-truth run (or fn, the composition from parts) in the device's place -> (out, the gradient of every leaf)."""
        leaves = [t.float().requires_grad_(True) for t in self.leaves]
        out = (fn or self.ref)(*leaves)
        return (out.detach().reshape(self.G.shape),) + torch.autograd.grad(out, leaves, self.G.float().reshape(-1))

    def rehearse(self):
        return self.price(*self.stand_in())


class ForwardCase:
    """One seeded case of an inference forward: `ref(dtype)` is the ground truth computed in `dtype`, G the tensor the result is
    shaped like; the subclass's __init__ sets `_refs` to None."""

    def refs(self):
        """(the fp64 ground truth, its fp32 run), computed once."""
        if self._refs is None:
            self._refs = (self.ref(torch.float64), self.ref(torch.float32))
        return self._refs

    def price(self, out, what=None):
        assert out.shape == self.G.shape and out.dtype == torch.float32, (self.name, out.shape, out.dtype)
        y64, y32 = self.refs()
        return _report(what or self.name, {"out": parity.close_fwd(out, y64, f"{what or self.name} out", y32)})

    def stand_in(self):
        """The fp32 ground-truth run in the device's place."""
        return self.refs()[1]

    def rehearse(self):
        return self.price(self.stand_in())


class DropoutChecks:
    """For a case under attention dropout with `mask` [E, H], pre-scaled: the rows whose entries are all dropped."""

    def all_dropped(self, min_entries=2):
        """bool [n_rows, H]: the row has at least min_entries entries and every one of them is dropped in that head."""
        kept = torch.zeros(self.shape[0], self.H).index_add(0, self.row, (self.mask != 0).float())
        deg = torch.bincount(self.row, minlength=self.shape[0])
        return (kept == 0) & (deg >= min_entries)[:, None]

    def check_all_dropped(self, out):
        gone = self.all_dropped()
        if bool(gone.any()):
            o = out.detach().cpu().reshape(self.shape[0], self.H, self.F)
            assert float(o[gone].abs().max()) == 0.0, f"{self.name}: a row whose entries are all dropped is an exact zero"


class ModuleCase:
    """A module with the op as `attend`: out and the gradients of its sum with respect to its inputs and weights, against the same
    module with the ground truth as `attend`, in fp64.  A subclass gives INPUTS (the attributes that hold the module's inputs), NAMES
    (its parameters, whose values are `weights`), GRADS (the names of all their gradients), `module(attend)`, `ref_attend` and G."""
    op = "module"

    @property
    def leaves(self):
        return [getattr(self, n) for n in self.INPUTS] + self.weights

    def ref(self, *leaves):
        """The module with the ground truth as `attend`, its parameters replaced by the weights among `leaves` (in their dtype)."""
        n = len(self.INPUTS)
        return torch.func.functional_call(self.module(self.ref_attend), dict(zip(self.NAMES, leaves[n:])), tuple(leaves[:n])).reshape(-1)

    def price(self, out, *grads):
        rep, _ = parity.check_autograd(out.reshape(-1), list(grads), self.ref, self.leaves, self.G, list(self.GRADS), self.name)
        return _report(self.name, rep)

    def rehearse(self):
        leaves = [t.float().requires_grad_(True) for t in self.leaves]
        out = self.ref(*leaves)
        return self.price(out.detach(), *torch.autograd.grad(out, leaves, self.G.float()))
