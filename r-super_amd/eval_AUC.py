"""python -m rsuper_amd.eval_AUC: the nine-threshold volumes and maximum probabilities of rsuper_train/eval_AUC.py over a tree of saved lesion
probabilities (`<case>/predictions_raw/<class>.npz`), measured on the device; writes tumor_detection_results_th0.1.csv ... _th0.9.csv.  The walk,
the flags and the CSV layout are test_with_reports.run's."""
from .test_with_reports import run


def main(argv=None):
    return run(argv, 'auc')


if __name__ == '__main__':
    main()
