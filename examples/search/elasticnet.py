"""
Searching the penalty: C x l1_ratio as ONE batched solve.

``LogisticRegression`` / ``LinearSVC`` take sklearn's ``penalty``
("l2" | "l1" | "elasticnet") and ``l1_ratio``; with ``lam = 1/(C n)`` the
L2 coefficient is ``(1 - l1_ratio) lam`` and the L1 coefficient
``l1_ratio lam``.  Both are per-column hyper-parameters of the batched
solver, so a grid over them costs what a grid over ``C`` alone costs:
every (candidate x fold) model is still one column of the same solve.
The L1 part is the cumulative-penalty update, so ``coef_`` holds exact
zeros — here 4 of 32 columns carry the signal and the other 28 drop out.
"""

import numpy as np
import torch

from skdist_amd import Cluster
from skdist_amd.distribute.search import DistGridSearchCV
from skdist_amd.models import LogisticRegression

rng = np.random.default_rng(0)
X = rng.standard_normal((4000, 32)).astype(np.float32)
z = X[:, :4] @ np.array([2.0, -2.0, 1.5, -1.5])
y = (z + 0.5 * rng.standard_normal(4000) > 0).astype(np.int64)

sc = Cluster()   # a GPU node's devices, or the local CPU fallback
print("device:", sc.device, "(HIP kernels)" if torch.cuda.is_available()
      else "(eager CPU path)")
gs = DistGridSearchCV(
    LogisticRegression(penalty="elasticnet", l1_ratio=0.5, epochs=20,
                       batch_size=256, random_state=0),
    {"C": [0.003, 0.03, 0.3], "l1_ratio": [0.0, 0.5, 1.0]},
    cv=3, sc=sc,
)
gs.fit(X, y)
print("best:", gs.best_params_, "CV accuracy:", round(gs.best_score_, 4))

for l1_ratio in (0.0, 0.5, 1.0):
    m = LogisticRegression(penalty="elasticnet", C=0.003, l1_ratio=l1_ratio,
                           epochs=20, batch_size=256, random_state=0)
    m.fit(X, y)
    print(f"C=0.003 l1_ratio={l1_ratio}: "
          f"{int((m.coef_ == 0).sum())} of 32 coefficients are exactly 0, "
          f"train accuracy {(m.predict(X) == y).mean():.3f}")

sparse = LogisticRegression(penalty="l1", C=0.003, epochs=20,
                            batch_size=256, random_state=0).fit(X, y)
assert (sparse.coef_[0, 4:] == 0).all() and (sparse.coef_[0, :4] != 0).all()
print("penalty='l1' keeps columns", np.flatnonzero(sparse.coef_[0]))
