"""The contract of include/memb_hip_cosmul.h restated on its own: a scalar loop over np.float32 values, one candidate and
one term at a time, written apart from memb_amd.reader.cosmul_scores_host; the float64 evaluation of the same formula the
rounding bound is measured against; and the k best by the score, which is the selection with a list of non-candidates
(analogies_reference.topk_excluding_by_the_contract) over the score matrix."""
import numpy as np

from analogies_reference import topk_excluding_by_the_contract

ONE = np.float32(1.0)
HALF = np.float32(0.5)
EPSILON = np.float32(0.000001)


def cosmul_score_of_one(cosines, negatives_from):
    """the float32 score of ONE candidate from the float32 cosines of a question's terms, the first `negatives_from` of them
    positive: every line one float32 operation"""
    num, den = ONE, ONE
    for index, cosine in enumerate(cosines):
        shifted = np.float32(ONE + np.float32(cosine))
        shifted = np.float32(shifted * HALF)
        if index < negatives_from:
            num = np.float32(num * shifted)
        else:
            den = np.float32(den * shifted)
    den = np.float32(den + EPSILON)
    return np.float32(num / den)


def cosmul_scores_by_the_contract(cosines, offsets, negatives_from):
    """float32 (Q, n): question q over the rows offsets[q] .. offsets[q + 1] of the float32 (T, n) matrix, the rows before
    negatives_from[q] positive"""
    cosines = np.ascontiguousarray(cosines, dtype=np.float32)
    questions = len(negatives_from)
    scores = np.zeros((questions, cosines.shape[1]), dtype=np.float32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
        for q in range(questions):
            begin, end = int(offsets[q]), int(offsets[q + 1])
            for column in range(cosines.shape[1]):
                scores[q, column] = cosmul_score_of_one(cosines[begin:end, column], int(negatives_from[q]) - begin)
    return scores


def cosmul_scores_in_float64(cosines, offsets, negatives_from):
    """the same formula over the same float32 cosines in float64, with float64(float32(1e-6))"""
    cosines = np.ascontiguousarray(cosines, dtype=np.float32).astype(np.float64)
    scores = np.zeros((len(negatives_from), cosines.shape[1]), dtype=np.float64)
    for q in range(len(negatives_from)):
        begin, split, end = int(offsets[q]), int(negatives_from[q]), int(offsets[q + 1])
        num = np.prod((1.0 + cosines[begin:split]) * 0.5, axis=0)
        den = np.prod((1.0 + cosines[split:end]) * 0.5, axis=0)
        scores[q] = num / (den + np.float64(EPSILON))
    return scores


def cosmul_topk_by_the_contract(cosines, offsets, negatives_from, k, excluded=None):
    """(values float32 (Q, k), positions int64 (Q, k)) of the score matrix"""
    return topk_excluding_by_the_contract(cosmul_scores_by_the_contract(cosines, offsets, negatives_from), k, excluded)


def questions_of(pairs):
    """(offsets int64 (Q + 1), negatives_from int64 (Q), T) of questions given as (P, N) pairs, laid end to end"""
    offsets, negatives_from = [0], []
    for positives, negatives in pairs:
        negatives_from.append(offsets[-1] + positives)
        offsets.append(offsets[-1] + positives + negatives)
    return np.array(offsets, dtype=np.int64), np.array(negatives_from, dtype=np.int64), offsets[-1]
