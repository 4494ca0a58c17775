"""
Multilabel tagging with DistOneVsRestClassifier (reference analog: the
``MultiLabelBinarizer`` route of skdist's DistOneVsRestClassifier, with
``max_negatives`` down-sampling the negatives of every label).

``y`` is a list of tag sets.  With ``sc=Cluster()`` and a native linear
estimator every tag trains as one column of a single batched solve: the
target and the train mask of every (row, tag) travel as bit planes, so
there is one dataset upload and one solve instead of one fit per tag, and
``predict`` is one GEMM plus a threshold.  ``max_negatives`` keeps all
positives of a tag and a capped sample of its negatives -- the same rows the
per-tag fits of the generic path (``sc=None``) train on.
"""

import numpy as np
from sklearn.metrics import f1_score

from skdist_amd import Cluster
from skdist_amd.distribute.multiclass import DistOneVsRestClassifier
from skdist_amd.models import LogisticRegression

rng = np.random.default_rng(0)
n, f, n_tags = 3000, 32, 12
X = rng.standard_normal((n, f)).astype(np.float32)
W = rng.standard_normal((f, n_tags))
# rare tags: about 1.5 per row, some rows with none
scores = X @ W + 0.5 * rng.standard_normal((n, n_tags))
Y = scores > np.quantile(scores, 1.0 - 1.5 / n_tags, axis=0)
names = np.array([f"tag{j:02d}" for j in range(n_tags)])
tags = [tuple(str(t) for t in names[row]) for row in Y]
print("rows without a tag:", sum(len(t) == 0 for t in tags),
      "| most tags on a row:", max(len(t) for t in tags))

sc = Cluster()
for max_negatives in (None, 0.3):
    clf = DistOneVsRestClassifier(
        LogisticRegression(epochs=30, batch_size=512, random_state=0),
        sc=sc, max_negatives=max_negatives, random_state=0)
    clf.fit(X, tags)
    pred = clf.predict(X)                      # list of tag tuples again
    ind = clf.mlb_.transform(pred)
    print(f"max_negatives={max_negatives}: micro-F1",
          round(f1_score(Y, ind, average="micro"), 4),
          "| first row:", pred[0], "truth:", tags[0])
