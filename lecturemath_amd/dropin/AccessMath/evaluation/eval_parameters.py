"""EvalParameters: the switches of the summary evaluation, with the release's names and default values
(AccessMath/evaluation/eval_parameters.py), read by AccessMath.evaluation.evaluator.Evaluator."""


class EvalParameters:
    # unique ground-truth CCs against the CCs of a summary's binary keyframes
    UniqueCC_global_tran_window = 10            # window of the keyframe-to-keyframe translation alignment
    UniqueCC_local_trans_window = 3             # extra displacement tried per CC pair (the device path takes up to 8)
    UniqueCC_min_translation_fscore = 0.3       # below it an alignment of consecutive keyframes is dropped
    UniqueCC_min_precision = [0.50, 0.65, 0.80, 0.95]
    UniqueCC_min_recall = [0.50, 0.65, 0.80, 0.95]
    UniqueCC_size_percentiles = [10, 25, 75]
    UniqueCC_min_align_recall = 0.05            # below it a ground-truth / summary keyframe pair is skipped

    UniqueCC_max_workers = 6                    # the release's process pool; unused here (one batched device call)

    # what the print_* reports show
    Report_Summary_Show_Counts = True
    Report_Summary_Show_AVG_per_frame = True
    Report_Summary_Show_Globals = True
    Report_Summary_Show_stats_per_size = True
